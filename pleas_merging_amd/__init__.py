"""MI355X-native PLeaS activation-matching + least-squares merging hot path.

Host side mirrors the reference's ``pleas.core`` / ``pleas.methods`` API; the
compute is done by hand-written gfx950 HIP kernels behind the C-ABI declared in
``include/pleas_hip.h`` (library ``pleas_merging_amd/csrc/libpleas_hip.so``).
"""
# Importing this package changes nothing in the process (rounds 1-4 set MIOPEN_DEBUG_CONV_WINOGRAD here): the k x k convolutions
# of the frozen source / twin forwards -- the only ones whose vendor kernels mattered for parity -- run on the library's own kernel
# since round 5 (methods/source_forward.py: SOURCE_CONV; PLEAS_SOURCE_CONV=vendor restores the vendor path).

__version__ = "0.6.0"
