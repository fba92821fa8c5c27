// Backward of the fused MAT-Dec shared actor (token-on-lane tiles, mat_actor_ct.hip) as its own translation unit:
// EIGHT waves per workgroup, two row tiles per wave at most, like the encoder / decoder backwards
// (mat_enc_ct_bwd.hip) — the 8-wave block mapping is what the private gradient copies' fragment order assumes.
#ifndef MDL_CT_BWD_NW
#define MDL_CT_BWD_NW 8
#endif
#define MDL_NW MDL_CT_BWD_NW
#if MDL_CT_BWD_NW == 8
#define MDL_MAXRT 2
#endif
#define MDL_CT_BWD_TU
#include "mat_actor_ct.hip"
