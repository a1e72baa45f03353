// What the test hooks of gemm_f32.hip and vae_debug.hip share.
#pragma once
#include "sln_common.h"
#include "sln_hip.h"

// fills v from the plain-C description; false when the view lacks what the coefficients `coef` (SLN_COEF_*) read out of it
bool sln_dbg_bn(const SlnDbgBn& d, int coef, BnView& v);
// leaf launches an engine issued so far (vae_engine.hip; read by sln_debug_vae_leaf_launches)
long sln_vae_engine_leaf_launches(const SlnVae* h);
// iterations whose wgrads ran as one mixed launch (vae_engine.hip; read by sln_debug_vae_tail_launches)
long sln_vae_engine_tail_launches(const SlnVae* h);
// fp16-MFMA Linear launches an engine issued so far (vae_engine.hip; read by sln_debug_vae_half_launches)
long sln_vae_engine_half_launches(const SlnVae* h);
// training iterations an engine captured into a graph so far (vae_engine.hip; read by sln_debug_vae_graph_captures)
long sln_vae_engine_graph_captures(const SlnVae* h);
