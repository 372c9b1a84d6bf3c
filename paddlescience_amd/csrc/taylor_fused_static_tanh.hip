// taylor_fused_static_tanh.hip -- the fused tile kernels of plans whose residual program is a compile-time table
// (csrc/epi_static.h, epi_static_programs.h), activation "tanh".
#ifndef PPSCI_SPLIT_CONST_VGPR
#define PPSCI_SPLIT_CONST_VGPR 1  // split constants in VGPRs, materialised once per kernel (ppsci_common.h)
#endif
#define PPSCI_ACT_ID PPSCI_ACT_TANH
#define PPSCI_FUSED_STATIC 1
// shape-specialised instantiations (taylor_fused.inc, D_RAW / M): two raw inputs, one output -- the scalar 2-D / 1-D + time PINNs
#define PPSCI_FUSED_SPEC_D_RAW 2
#define PPSCI_FUSED_SPEC_M 1
// ... and their KEEP twins where the carve-up fits half a CU: L = 3, 4, 5 of the stream sets with S <= 4
#ifndef PPSCI_FUSED_KEEP_PLANES
#define PPSCI_FUSED_KEEP_PLANES 1
#endif
#define PPSCI_FUSED_RUN_NAME ppsci_fused_static_run_tanh
#include "taylor_fused.inc"
