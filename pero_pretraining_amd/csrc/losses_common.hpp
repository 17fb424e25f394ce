// Host-side launch helpers shared by the loss kernels (losses.hip, ntxent_ragged.hip) and, through ctc_common.hpp, by the CTC sources.
#pragma once
#include "common.hpp"
#include <initializer_list>

#define DISPATCH_T(dtype, NAME, ...)                                                              \
  do {                                                                                            \
    if (dtype == PERO_F32) { NAME(float, __VA_ARGS__); }                                          \
    else if (dtype == PERO_BF16) { NAME(bf16raw, __VA_ARGS__); }                                  \
    else PERO_REQUIRE(false, "bad dtype");                                                        \
  } while (0)

// 16-byte row accesses are possible when every row starts 16-byte aligned
static inline bool v8_ok(int64_t d, int dtype, std::initializer_list<const void*> ptrs) {
  const int esz = dtype == PERO_F32 ? 4 : 2;
  if (d % 8 || (d * esz) % 16) return false;
  for (const void* q : ptrs) if (!aligned16(q)) return false;
  return true;
}
