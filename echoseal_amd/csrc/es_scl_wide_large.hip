// es_scl_wide_large.hip -- the lane-per-path list decoder (es_scl_wide.hip) for lists of 257..1024 paths: its 512- and 1024-lane
// instantiations, for the reference's code and for run-time K, and their launcher es_launch_scl_wide_large (es_launch_scl_wide hands
// such lists over).  A unit of its own so that the instantiations of lists up to 256 paths compile exactly as they do without these.
#define ES_WIDE_LARGE_TU 1
#include "es_scl_wide.hip"
