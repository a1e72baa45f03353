// What the test hooks of gemm_f32.hip and vae_debug.hip share.
#pragma once
#include "sln_common.h"
#include "sln_hip.h"

// fills v from the plain-C description; false when the view lacks what the coefficients `coef` (SLN_COEF_*) read out of it
bool sln_dbg_bn(const SlnDbgBn& d, int coef, BnView& v);
