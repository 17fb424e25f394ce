// Shared by the two kernels on the eight-phase schedule: gemm_bf16_e256 (gemm_e.hip, where the schedule is described) and gemm_bf16_n512
// (gemm_n.hip): the epilogue modes, the uncounted loads / stores and their waits, the LDS-DMA addressing and
// the primitives of a phase.
#pragma once
#include "gemm_common.hpp"

#define E_BK 64
#define E_HALF 16384               // half tile: 128 rows x 64 k (bf16)

// epilogue modes
#define EP_PLAIN 0       // bias
#define EP_RELU 1        // bias, ReLU
#define EP_RESID 2       // bias, + residual (bf16 rows of C's shape)
#define EP_RELU_BITS 3   // bias, ReLU, `gate` receives the bit mask (stored C > 0)
#define EP_GATE_BITS 4   // `gate` bit mask applied; with PERO_GEMM_COLSUM the column sums of the stored result are added to `bias`
#define EP_ROWDOT 6      // `bias`[m][n / 128] += row dots of the stored result with `gate` (bf16 rows of C's shape)
#define EP_SPLITK 7      // f32 C += partial product of ONE k-slice (atomics): one work item (tile, k-slice) per workgroup, not persistent
#define EP_RESID_LN 8    // (gemm_bf16_n512 only) bias, + residual -> y stored; LayerNorm of the stored rows -> t, mean, rstd (LnP)
#define EP_RESID_LN_T 9  // the same without the stores of y (the backward reads t: pero_layernorm_bwd_out): the epilogue's counted waits differ
#define EP_RESID_LNB 10  // (gemm_bf16_n512 only) input gradient of a Linear + residual gradient = dt, rows complete -> LayerNorm BACKWARD of the upstream norm
                         // in the epilogue (from its output t and rstd, pero_layernorm_bwd_out's arithmetic): dx stored, dt never; column sums -> LnP.work
// second argument of gemm_bf16_n512: what the LayerNorm epilogue writes and reads beside GemmP
struct LnP { void* t; long long ldt; float* mean; float* rstd; const float* gamma; const float* beta; float eps; float* work; };
typedef float ef2v __attribute__((ext_vector_type(2)));
#define E_BLOAD4(dst_, voff_, rs_, soff_, imm_) \
  asm volatile("s_nop 4\n\tbuffer_load_dword %0, %1, %2, %3 offen offset:%4" : "=v"(dst_) : "v"(voff_), "s"(rs_), "s"(soff_), "i"(imm_) : "memory")

typedef int ei4v __attribute__((ext_vector_type(4)));
typedef short es2v __attribute__((ext_vector_type(2)));
typedef unsigned short eus2v __attribute__((ext_vector_type(2)));
// two bf16 in a dword: ReLU as a signed 16-bit maximum with zero; (half != 0) per half for halves that are +0 or positive
__device__ __forceinline__ unsigned epk_relu(unsigned v) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(es2v, v), (es2v){0, 0}));
}
// acc + a.lo * b.lo + a.hi * b.hi of two bf16 pairs (v_dot2c_f32_bf16)
__device__ __forceinline__ float edot2(unsigned a, unsigned b, float acc) {
  typedef __bf16 eb2v __attribute__((ext_vector_type(2)));
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(eb2v, a), __builtin_bit_cast(eb2v, b), acc, false);
}
__device__ __forceinline__ unsigned epk_nonzero(unsigned v) {   // (hipcc turns the vector minimum into compares and selects: asm)
  unsigned r;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(v), "s"(0x00010001u));
  return r;
}
typedef unsigned eu4v __attribute__((ext_vector_type(4)));
typedef unsigned eu2v __attribute__((ext_vector_type(2)));

// per-thread byte offset of its two LDS-DMA pieces inside a half tile's source (constant over the whole kernel).
// Rows of the half tiles are INTERLEAVED so that a wave's outputs are contiguous in memory: row r of A half h is row
// (r >> 6) * 128 + 64 h + (r & 63) of the tile, row r of B half h is column (r >> 5) * 64 + 32 h + (r & 31).
template <bool TR, bool ISA>
__device__ __forceinline__ unsigned elane_off(long long ld, int tid) {
  if (!TR) {  // K-contiguous operand: piece = 8 rows x 128 B; LDS slot (tid & 7) of row r holds chunk slot ^ (r & 7)
    const int r = tid >> 3, chunk = (tid & 7) ^ (r & 7);
    const int g = ISA ? r : ((r >> 5) * 64 + (r & 31));
    return (unsigned)((g * ld + chunk * 8) * 2);
  } else {    // K-major operand: piece = 4 k-rows x 256 B; 32-byte blocks of a k-row XORed with fk(krow)
    const int krow = tid >> 4, slot = tid & 15;
    const int c = ((((slot >> 1) ^ fk(krow)) << 1) | (slot & 1)) * 8;
    const int g = ISA ? ((c >> 6) * 128 + (c & 63)) : ((c >> 5) * 64 + (c & 31));
    return (unsigned)((krow * ld + g) * 2);
  }
}
// byte steps of an operand's half-tile stream (uniform): tile origin t0, K-tile u, half h, second piece
template <bool TR, int HS>
struct EStep {
  long long tile, ktile, half, piece;
  __device__ __forceinline__ EStep(long long ld) {
    if (!TR) { tile = ld * 2; ktile = E_BK * 2; half = HS * ld * 2; piece = 128 * ld * 2; }
    else { tile = 2; ktile = E_BK * ld * 2; half = HS * 2; piece = 32 * ld * 2; }
  }
};
__device__ __forceinline__ void eglds2(const unsigned char* base, long long piece, unsigned off, unsigned char* dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + off),
                                   (__attribute__((address_space(3))) void*)(dst), 16, 0, 0);
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + piece + off),
                                   (__attribute__((address_space(3))) void*)(dst + 8192), 16, 0, 0);
}
// buffer descriptor from uniform values (raw buffer, 32-bit offsets, no bounds beyond `bytes`)
__device__ __forceinline__ ei4v ersrc(const void* base, unsigned bytes) {
  const unsigned long long b = (unsigned long long)base;
  ei4v r;
  r[0] = (int)(unsigned)b; r[1] = (int)(unsigned)((b >> 32) & 0xffffu); r[2] = (int)bytes; r[3] = 0x00020000;
  return r;
}
// loads the compiler does not see (no wait of its own, not in its vmcnt bookkeeping): waited for by E_WAIT* below
#define E_BLOAD16(dst_, voff_, rs_, soff_, imm_) \
  asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(dst_) : "v"(voff_), "s"(rs_), "s"(soff_), "i"(imm_) : "memory")
#define E_BLOAD8(dst_, voff_, rs_, soff_, imm_) \
  asm volatile("s_nop 4\n\tbuffer_load_dwordx2 %0, %1, %2, %3 offen offset:%4" : "=v"(dst_) : "v"(voff_), "s"(rs_), "s"(soff_), "i"(imm_) : "memory")
// 16-byte store: its data registers are rewritten by the next unit right behind it.  hipcc (ROCm 7.2) pads that hazard only for
// a constant soffset; with the row offset in an SGPR the store sent stale dwords for some lanes (measured: lanes 12-15 of the
// second data dword) - the wait states are in the string
// ... and IN FRONT of it: the compiler does not look into the string, so nothing keeps a v_readlane_b32 that restores a spilled SGPR (the row
// offset, the descriptor) apart from the store that reads it - a vector-ALU write of an SGPR needs five wait states before a vector-memory
// instruction uses it, and a store issued too early takes the SGPR's OLD value: rows of the LayerNorm epilogue (87 spilled SGPRs) landed in
// other row groups, run-to-run different (E_BLOAD16 has had its s_nop 4 for the same reason)
#define E_BSTORE16(src_, voff_, rs_, soff_, imm_) \
  asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, %3 offen offset:%4\n\ts_nop 2" :: "v"(src_), "v"(voff_), "s"(rs_), "s"(soff_), "i"(imm_) : "memory")
#define E_WAIT8(n_, r_) \
  asm volatile("s_waitcnt vmcnt(%8)" : "+v"(r_[0]), "+v"(r_[1]), "+v"(r_[2]), "+v"(r_[3]), "+v"(r_[4]), "+v"(r_[5]), "+v"(r_[6]), "+v"(r_[7]) : "i"(n_) : "memory")
#define E_WAIT4(n_, r_) \
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(r_[0]), "+v"(r_[1]), "+v"(r_[2]), "+v"(r_[3]) : "i"(n_) : "memory")


// ---- the primitives of a phase.  All macros: every kernel's machine code is pinned byte for byte, and written as inline functions the two
// address computations at the end came out with other operand orders / another instruction schedule in some instantiations.
// raw barrier the compiler moves nothing across
#define E_BAR()                                  \
  __builtin_amdgcn_sched_barrier(0);             \
  __builtin_amdgcn_s_barrier();                  \
  __builtin_amdgcn_sched_barrier(0);
// the phase's fragment reads have arrived
#define E_LGKM0()                                          \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       \
  __builtin_amdgcn_sched_barrier(0);
// counted wait on the one in-order counter of LDS-DMA, loads and stores: at most n_ of them stay in flight
#define E_VMCNT(n_) asm volatile("s_waitcnt vmcnt(%0)" :: "i"(n_) : "memory")
// the tile's 128 accumulator registers cleared (the first K-tile's MFMAs then take the zeros as an inline constant: no moves)
#define E_ACC_ZERO()                                                     \
  _Pragma("unroll") for (int ha_ = 0; ha_ < 2; ha_++)                    \
  _Pragma("unroll") for (int hb_ = 0; hb_ < 2; hb_++)                    \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++)                       \
  _Pragma("unroll") for (int j_ = 0; j_ < 2; j_++) acc[ha_][hb_][i_][j_] = (f4v){0.f, 0.f, 0.f, 0.f}
// one phase's 16 MFMAs: the kernel's acc[HA_][HB_] += its A fragments fa x the B fragments F_, operands swapped (a lane owns 4 consecutive
// output columns of one row)
#define E_MFMA(HA_, HB_, F_)                                                                                              \
  __builtin_amdgcn_s_setprio(1);                                                                                          \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; s_++)                                                                        \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++)                                                                        \
  _Pragma("unroll") for (int j_ = 0; j_ < 2; j_++)                                                                        \
    acc[HA_][HB_][i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F_[j_][s_], fa[i_][s_], acc[HA_][HB_][i_][j_], 0, 0, 0); \
  __builtin_amdgcn_s_setprio(0);
// fragment read offset of a lane inside a K-contiguous half-tile image [128 rows][128 B]: row (lane & 15) of a 16-row group, 16-byte chunk
// (4 s + (lane >> 4)) ^ (row & 7) for s = 0; s = 1 is the offset ^ 64
#define E_FRAG_OFF(lane_) ((unsigned)(((lane_) & 15) * 128 + (((((lane_) >> 4)) ^ ((lane_) & 7)) << 4)))
// Tile id of workgroup place T of a persistent grid (a multiple of 8) over nt = 8 q8 + r8 tiles.  Workgroup T runs on XCD T & 7: every XCD
// takes a CONTIGUOUS range of tile ids (the first r8 XCDs one more), so that the tiles which share operand panels meet in one L2;
// loc = the place inside the XCD's range (T >> 3, or what the kernel's walk makes of it).
#define E_XCD_TILE(xcd_, loc_, q8_, r8_) (((xcd_) < (r8_) ? (xcd_) * ((q8_) + 1) : (r8_) * ((q8_) + 1) + ((xcd_) - (r8_)) * (q8_)) + (loc_))
