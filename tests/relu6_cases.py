"""Shapes and networks of the ReLU6 tests, shared by tests/test_relu6_host.py and tests/test_hip_relu6.py (importing this file
needs no torch)."""

# (n, C, inner) of the elementwise passes: the scalar path (inner % 4 != 0) and the 16-byte path
BN_ACT_SHAPES = [(2, 5, 63), (2, 8, 16)]

# one geometry per epilogue branch of csrc/conv_fwd.hip: (N, Cin, H, W, Cout, K, stride, pad)
CONV_CASES = {
    "vector": (2, 32, 8, 8, 40, 1, 1, 0),       # Ho * Wo % 4 == 0
    "scalar": (1, 16, 7, 7, 24, 3, 1, 1),       # 49 output pixels
    "stem": (2, 3, 9, 9, 8, 3, 2, 1),           # few input channels, stride 2, 25 output pixels
}

# tests/depthwise_cases.CASES entries of the depthwise epilogue: odd and unaligned, stride 2, K = 5, more than one workgroup
DW_CASES = (0, 1, 3, 8)

# values planted into one channel that runs with scale 1 and shift 0 (nextafter(6, +-inf) are added by the test)
EDGE_VALUES = (float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 6.0, 6.5, -1e-30)

SMALL_SETTING = [[1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 2, 1]]
SMALL_INPUT = (4, 3, 32, 32)


def small_mobilenet(classes: int = 10):
    """The small inverted-residual network of the end-to-end tests: a stem, a t = 1 block with a residual add, four expanding
    blocks (one of stride 2, two with a residual add), the 1 x 1 head convolution, pool, dropout, fc."""
    from pleas_merging_amd.mobilenet import mobilenet_v2

    return mobilenet_v2(num_classes=classes, width_mult=0.25, inverted_residual_setting=SMALL_SETTING)


def relu_twin(model):
    """A deep copy of ``model`` with every ``nn.ReLU6`` replaced by an ``nn.ReLU`` of the same ``inplace``."""
    import copy

    from torch import nn

    twin = copy.deepcopy(model)
    for parent in list(twin.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, nn.ReLU6):
                setattr(parent, name, nn.ReLU(inplace=child.inplace))
    return twin


def out_of_place(model):
    """A deep copy of ``model`` whose activation modules have ``inplace=False``."""
    import copy

    twin = copy.deepcopy(model)
    for m in twin.modules():
        if hasattr(m, "inplace"):
            m.inplace = False
    return twin
