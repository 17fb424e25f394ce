// Line augmentation fused into batch collation (the reference augments on the host, in the dataset:
// common/dataset.py:92-96, 247-254, an opaque `self.augmentations(image=image)` per decoded line).
//
// The second form of stack_lines_k (collate.hip): the same ragged upload in, the same padded (B, H, Wt, C) u8 batch out, each
// output byte written exactly once - but a byte inside the line's span is a bilinear sample of the line at a warped source
// position, sent through a per-line tone curve and given hashed noise.  The transform keeps the width: line b still occupies
// columns [left_px, left_px + w) and everything outside is zero, so masks, labels and shifts do not know about it.  Integer
// arithmetic only, every product i32 x i32 -> i64, every index clamped: bit-reproducible from the formulas of include/pero_hip.h,
// which tests/augment_ref.py restates.
#include "common.hpp"

__device__ __forceinline__ unsigned fmix32(unsigned h) {  // murmur3's finaliser
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Eight bytes from any address (the device runs with unaligned global access; one global_load_dwordx2).
__device__ __forceinline__ unsigned long long load8(const unsigned char* p) {
  unsigned long long q;
  __builtin_memcpy(&q, p, 8);
  return q;
}

// One thread produces 16 consecutive output bytes of row (b, y) with one uint4 store, so a wave stores 1 KiB contiguously like
// stack_lines_k.  It walks the PIXELS that overlap its 16 bytes (a walk over the bytes would evaluate the geometry at every byte
// of a wave: for C = 3 the lanes begin their pixels at different bytes): per pixel the geometry once, then two 8-byte loads - the
// taps (y0, x0), (y0, x1) and (y1, x0), (y1, x1) are neighbours in memory, 2 C <= 8 bytes per row, because x1 is x0 + 1 or,
// where the clamp made them equal, fx is set to 0 and the second tap's value does not matter.  A load may run up to 7 bytes past
// the line, into the next line or the buffer's 8 bytes of slack.  Neighbouring lanes sample neighbouring source pixels (the
// displacement field is smooth), so a wave's loads fall into a few cache lines of a line that stays in L2 (at most 245 KB).
// b, and with it every per-line parameter, is uniform in the block.
template <int C>
__global__ __launch_bounds__(128) void augment_stack_lines_k(const unsigned char* packed, const int64_t* off, const int* widths,
                                                             const int* left_px, const int* params, const int* knots,
                                                             const unsigned char* lut, unsigned char* out, int H, long long row_bytes,
                                                             long long chunks_per_row, int NK, int knot_shift) {
  constexpr int NP = 16 % C ? (16 + C - 2) / C + 1 : 16 / C;  // pixels that can overlap 16 bytes: 16, 8, 6, 4
  const long long chunk = (long long)blockIdx.x * 128 + threadIdx.x;
  if (chunk >= chunks_per_row) return;
  const int y = blockIdx.y, b = blockIdx.z;
  const int w = widths[b];
  const long long lo = (long long)left_px[b] * C, hi = lo + (long long)w * C;  // line span inside the row, in bytes
  const long long j0 = chunk * 16;
  const long long out_index = ((long long)b * H + y) * row_bytes + j0;          // of this thread's first byte in the batch
  unsigned char* dst = out + out_index;
  if (j0 + 16 <= lo || j0 >= hi) {
    *(uint4*)dst = make_uint4(0, 0, 0, 0);
    return;
  }
  const int* p = params + (long long)b * PERO_AUGMENT_PARAMS;
  const int sy = p[0], ty = p[1], slope = p[2], slant = p[3], noise_amp = p[4];
  const unsigned seed_lo = (unsigned)p[5], seed_hi = (unsigned)p[6];
  const int* ky = knots + (long long)b * 2 * NK;
  const int* kx = ky + NK;
  const unsigned char* line = packed + off[b];
  const unsigned char* tone = lut ? lut + (long long)b * C * 256 : nullptr;
  const int K = 1 << knot_shift;
  const int cy = (H - 1) * 128, xc = w / 2;
  const int yrel = (y << 8) - cy;                                                // |yrel| < 2^24: H < 65536
  const long long ys_line = (long long)cy + (((long long)yrel * sy) >> 8) + ty;  // the part of ys that does not depend on x
  const long long xs_line = ((long long)yrel * slant) >> 8;
  const long long pitch = (long long)w * C;                                      // of the line's rows in `packed`

  const long long first = j0 > lo ? j0 : lo;       // first line byte of this chunk
  const int x_first = (int)((first - lo) / C);     // its pixel, line-local
  const int k_first = (int)(lo - j0) + x_first * C;  // position of that pixel's channel 0 in the chunk: in (-C, 16)
  unsigned long long acc_lo = 0, acc_hi = 0;       // bytes 0-7 and 8-15
#pragma unroll
  for (int i = 0; i < NP; i++) {
    const int x = x_first + i, k = k_first + i * C;
    if (x >= w || k >= 16) continue;
    const int kj = clampi(x >> knot_shift, 0, NK - 2), t = x & (K - 1);
    const long long dy = ((long long)ky[kj] * (K - t) + (long long)ky[kj + 1] * t) >> knot_shift;
    const long long dx = ((long long)kx[kj] * (K - t) + (long long)kx[kj + 1] * t) >> knot_shift;
    const long long ys = ys_line + (long long)slope * (x - xc) + dy;
    const long long xs = ((long long)x << 8) + xs_line + dx;
    // a source position further than one pixel outside the line clamps like the position one pixel outside: both taps on the edge
    const int yi = (int)(clampll(ys, -256, (long long)H << 8) >> 8), xi = (int)(clampll(xs, -256, (long long)w << 8) >> 8);
    const int y0 = clampi(yi, 0, H - 1), y1 = clampi(yi + 1, 0, H - 1), x0 = clampi(xi, 0, w - 1), x1 = clampi(xi + 1, 0, w - 1);
    const unsigned fy = (unsigned)ys & 255, fx = x1 == x0 ? 0 : (unsigned)xs & 255;
    const unsigned long long q0 = load8(line + y0 * pitch + (long long)x0 * C), q1 = load8(line + y1 * pitch + (long long)x0 * C);
#pragma unroll
    for (int c = 0; c < C; c++) {
      const int kc = k + c;
      if (kc < 0 || kc >= 16) continue;
      const unsigned p00 = (unsigned)(q0 >> (8 * c)) & 255, p01 = (unsigned)(q0 >> (8 * (C + c))) & 255;
      const unsigned p10 = (unsigned)(q1 >> (8 * c)) & 255, p11 = (unsigned)(q1 >> (8 * (C + c))) & 255;
      unsigned v = ((p00 * (256 - fx) + p01 * fx) * (256 - fy) + (p10 * (256 - fx) + p11 * fx) * fy + 32768) >> 16;
      if (tone) v = tone[c * 256 + v];
      if (noise_amp != 0) {
        const unsigned long long idx = (unsigned long long)(out_index + kc);
        const unsigned h = fmix32(fmix32((unsigned)idx ^ seed_lo) ^ (unsigned)(idx >> 32) ^ seed_hi);
        const int s = (int)((h & 255) + ((h >> 8) & 255) + ((h >> 16) & 255) + (h >> 24)) - 510;
        v = (unsigned)clampi((int)v + (int)(((long long)s * noise_amp + 32768) >> 16), 0, 255);  // the noise is below 2^24
      }
      const unsigned long long placed = (unsigned long long)v << (8 * (kc & 7));
      acc_lo |= kc < 8 ? placed : 0;
      acc_hi |= kc < 8 ? 0 : placed;
    }
  }
  *(uint4*)dst = make_uint4((unsigned)acc_lo, (unsigned)(acc_lo >> 32), (unsigned)acc_hi, (unsigned)(acc_hi >> 32));
}

extern "C" int pero_augment_stack_lines(const void* packed, const int64_t* offsets, const int32_t* widths, const int32_t* left_px,
                                        const int32_t* params, const int32_t* knots, const uint8_t* lut, void* out, int64_t B,
                                        int64_t H, int64_t Wt, int64_t C, int64_t P, int64_t knot_shift, void* stream) {
  PERO_REQUIRE(packed && offsets && widths && left_px && params && knots && out, "pero_augment_stack_lines: null pointer");
  PERO_REQUIRE(B > 0 && B < 65536 && H > 0 && H < 65536 && C > 0 && C <= 4 && Wt > 0 && Wt < (1LL << 24),
               "pero_augment_stack_lines: bad sizes");
  PERO_REQUIRE(P == PERO_AUGMENT_PARAMS, "pero_augment_stack_lines: params must have %d columns (P = %lld)", PERO_AUGMENT_PARAMS,
               (long long)P);
  PERO_REQUIRE(knot_shift >= 3 && knot_shift <= 8, "pero_augment_stack_lines: knot_shift must be in [3, 8] (%lld)",
               (long long)knot_shift);
  PERO_REQUIRE((Wt * C) % 16 == 0 && aligned16(out),
               "pero_augment_stack_lines: padded rows must be 16-byte multiples (Wt*C = %lld)", (long long)(Wt * C));
  const long long row_bytes = Wt * C, chunks = row_bytes / 16;
  const dim3 grid((unsigned)((chunks + 127) / 128), (unsigned)H, (unsigned)B);
#define PERO_AUGMENT_LAUNCH(C_)                                                                                                    \
  hipLaunchKernelGGL(augment_stack_lines_k<C_>, grid, dim3(128), 0, (hipStream_t)stream, (const unsigned char*)packed, offsets,    \
                     widths, left_px, params, knots, lut, (unsigned char*)out, (int)H, row_bytes, chunks,                          \
                     (int)(Wt >> knot_shift) + 2, (int)knot_shift)
  switch (C) {
    case 1: PERO_AUGMENT_LAUNCH(1); break;
    case 2: PERO_AUGMENT_LAUNCH(2); break;
    case 3: PERO_AUGMENT_LAUNCH(3); break;
    default: PERO_AUGMENT_LAUNCH(4); break;
  }
#undef PERO_AUGMENT_LAUNCH
  PERO_CHECK_LAUNCH("pero_augment_stack_lines");
  return PERO_OK;
}
