from pleas_merging_amd.core.solvers import *  # noqa: F401,F403
from pleas_merging_amd.core.solvers import scipy_solve_lsa, hip_solve_lsa  # noqa: F401
from pleas_merging_amd.core.solvers import (hip_solve_minimax_assignment, host_solve_minimax_assignment,  # noqa: F401
                                            scipy_solve_minimax_assignment)
