#include "ipdm_common.h"
extern "C" int ipdm_abi_version(void) { return IPDM_ABI_VERSION; }
extern "C" const char* ipdm_build_arch(void) { return "gfx950"; }
extern "C" int ipdm_mask_layouts(void) { return IPDM_MASK_LINES | IPDM_MASK_2D; }
