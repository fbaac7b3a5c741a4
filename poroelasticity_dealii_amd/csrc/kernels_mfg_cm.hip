// The general cell-loop kernels with per-cell moduli (poro_ctx_set_cell_moduli): kernels_mfg.hip compiled with its static switch.  A translation unit of its own, so that
// the constant-moduli kernels of kernels_mfg.hip keep their names, their number and their code.
#define PORO_MFG_CELL_MODULI 1
#include "kernels_mfg.hip"
