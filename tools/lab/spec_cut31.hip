// A deliberately wrong spectrometer for tests/test_gpu_spec.py to notice (profiles/r21/LAB.md): the
// product's kern_spec.hip with its sub-blocks cut every 31 frames instead of 32.  Every access stays in
// bounds (the scratch is sized by the same constant); only the order of the sums changes.  Linked into
// tools/_build/libsdsp_spec_cut31.so by tools/lab.mk, never into libsdsp.so.
#define SDSP_SPEC_SUB 31
#include "kern_spec.hip"
