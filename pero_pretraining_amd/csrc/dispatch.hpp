// Host-side launch helpers of the typed entry points: the runtime dtype becomes an element type, a runtime bool becomes a compile-time
// constant, so that an entry point writes its hipLaunchKernelGGL argument list once:
//   PERO_REQUIRE(with_elem(dtype, [&](auto t) { using T = decltype(t); with_flag(v8, [&](auto V) {
//     hipLaunchKernelGGL((k<T, decltype(V)::value>), grid, block, 0, st, (const T*)x, ...); }); }), "pero_x: bad dtype");
#pragma once
#include "common.hpp"
#include <initializer_list>
#include <type_traits>

// f(T()) with T = float for PERO_F32, bf16raw for PERO_BF16; any other dtype calls nothing and returns false
template <typename F>
static inline bool with_elem(int dtype, F&& f) {
  if (dtype == PERO_F32) { f(float()); return true; }
  if (dtype == PERO_BF16) { f(bf16raw()); return true; }
  return false;
}
// f(std::true_type()) or f(std::false_type())
template <typename F>
static inline void with_flag(bool flag, F&& f) {
  if (flag) f(std::true_type()); else f(std::false_type());
}

// 16-byte row accesses are possible when every row starts 16-byte aligned
static inline bool v8_ok(int64_t d, int dtype, std::initializer_list<const void*> ptrs) {
  const int esz = dtype == PERO_F32 ? 4 : 2;
  if (d % 8 || (d * esz) % 16) return false;
  for (const void* q : ptrs) if (!aligned16(q)) return false;
  return true;
}
