// The library's run-time options (pero_set_option): THE list - name, default, meaning.  The struct's fields and the name table of
// pero_set_option (api.hip, where the one instance lives) are both made from it; the code reads g_opt.<name>.  Process-wide, not meant to
// be changed while products are in flight (include/pero_hip.h).
#pragma once

#define PERO_OPTIONS(X)                                                                                                                  \
  X(gemm_policy, 0, "tile-kernel family (table above gemm_plan in gemm.hip): 0 = auto, 1 = 128x128x64 persistent, 4 = gemm_bf16_o128, 7 = gemm_bf16_r256, 20 = gemm_bf16_e256") \
  X(attn_bwd_pair, 1, "the attention backward with D handed in runs as one launch")                                                      \
  X(attn_order, 32, "dispatch order of the paired backward's blocks (attn_bwd_pair_k); 0 = a unit's four blocks side by side")           \
  X(splitk_workspace, 1, "split-K of gemm_bf16_e256 leaves partial tiles in the caller's workspace; 0: f32 atomics")                     \
  X(splitk_table, 1, "unaligned slice counts hand their work items out XCD by XCD; 0: plain item order")                                 \
  X(gemm_nw, 0, "1: N = 512 stored products with the plain / residual epilogue on the row-complete tile gemm_bf16_n512")                 \
  X(gemm_e_walk, 1, "stored K <= 512 products walk several N-tiles of a row panel one after the other; 0: all side by side")             \
  X(gemm_e256_min, 192, "auto: stored products with at least this many 256x256 tiles take the eight-phase kernel (0 = never)")           \
  X(gemm_e_splitk_min, 4, "... and split-K products (reduction >= 32768 rows) with at least this many output tiles")                     \
  X(splitk_xcd, 1, "gemm_bf16_o128: one k-slice per XCD where the slice count allows it")                                                \
  X(splitk_nearest, 0, "split-K of the 128x128 kernels: slice counts >= 8 round to the nearest multiple of 8 instead of up")             \
  X(splitk_items, 512, "split-K of the 128x128 kernels aims at this many work items (<= 0 stores 512)")

struct PeroOptions {
#define X(name_, default_, meaning_) int name_ = default_;
  PERO_OPTIONS(X)
#undef X
};
extern PeroOptions g_opt;
