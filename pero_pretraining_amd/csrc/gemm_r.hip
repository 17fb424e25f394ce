// 256 x 128 x 32 bf16 tile GEMM, 8 waves (4 along M x 2 along N, 64 x 64 each), two workgroups per CU (16 waves, <= 128
// VGPRs).  Same structure as gemm_bf16_s128 (gemm_s.hip) with a taller tile: 3 LDS-DMA instructions per wave and k-step
// instead of 4 for the same 16 MFMAs, and 25 % fewer L2->LDS bytes per flop.
#include "gemm_common.hpp"

#define R_BM 256
#define R_BN 128
#define R_BK 32
#define R_ABYTES (256 * 32 * 2)      // 16 KiB A tile
#define R_OPBYTES R_ABYTES
#define R_BBYTES (128 * 32 * 2)      // 8 KiB B tile
#define R_BUFBYTES (R_ABYTES + R_BBYTES)   // 24 KiB per stage
#define R_EPI_PITCH 528                // f32 staging pitch (128 * 4 + 16)
// 2 stages (48 KiB): a 3-stage ring (72 KiB, two workgroups = 144 KiB) was 1.3 % faster alone but leaves no LDS for the
// weight-gradient products that run beside it on the side streams: the step lost 3 % (tools/step_ab2.py).
// R_ASLOTS slots for the A operand (the streamed one) + two for B: with three A slots the A DMA has two stages to land
// (gemm_v.hip); 3 x 16 + 2 x 8 = 64 KiB.
#ifndef R_ASLOTS
#define R_ASLOTS 3
#endif
#define R_LDS_BYTES (R_ASLOTS * R_ABYTES + 2 * R_BBYTES)   // >= 64-row f32 staging of 33792 B; two workgroups per CU

// K-contiguous image [128 rows][32 k] = 64-byte rows, 4 chunks of 16 B, four rows per 256-byte bank row.  A
// ds_read_b128 is served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... (MI355X_MICROARCH.md, LDS):
// each holds the 16 rows of the fragment with chunk c for rows {0-3, 12-15} and chunk c^1 for rows {4-11}.  XORing
// the chunk with g(row) = [0,2,3,1][(row >> 2) & 3] puts them on 16 distinct 16-byte slots (SQ_LDS_BANK_CONFLICT
// fell from 0.44 of the LDS-active cycles with the naive (row >> 2) & 3 XOR to 0).
__device__ __forceinline__ int rg(int row) { return (0x78 >> (((row >> 2) & 3) << 1)) & 3; }
__device__ __forceinline__ bf8v rfrag_rowmajor(const unsigned char* base, int row, int lane) {
  const int r = row + (lane & 15);
  const int chunk = lane >> 4;
  return *(const bf8v*)(base + r * 64 + ((chunk ^ rg(r)) << 4));
}
// K-major image [32 k-rows][COLS cols] (COLS * 2-byte rows), 32-byte blocks XORed with fk(krow) (low 3 bits)
template <int COLS>
__device__ __forceinline__ bf8v rfrag_kmajor(const unsigned char* base, int col, int lane) {
  const int i = lane & 15;
  const int krow = 8 * (lane >> 4) + (i >> 2);
  const unsigned char* a = base + krow * (COLS * 2) + ((((col >> 4) ^ fk(krow))) << 5) + 8 * (i & 3);
  s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s4v, a));
  s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s4v, a + 4 * (COLS * 2)));
  typedef short s8v __attribute__((ext_vector_type(8)));
  s8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf8v, v);
}
// operand tile of ROWS (256 for A, 128 for B) x 32 k: ROWS/16 pieces of 1 KiB, 8 waves -> ROWS/128 pieces per wave
template <bool TR, int ROWS>
__device__ __forceinline__ void rstage_glds(const bf16raw* X, long long ld, long long tile0, long long k0,
                                            unsigned char* lds_base, int tid) {
  unsigned char* dst = lds_base + (tid >> 6) * 1024;
  if (!TR) {  // piece = 16 rows x 64 B: thread -> row (tid >> 2) + 128 i, LDS slot tid & 3
    const int row = tid >> 2, chunk = (tid & 3) ^ rg(row);
    const bf16raw* p = X + (tile0 + row) * ld + k0 + chunk * 8;
#pragma unroll
    for (int i = 0; i < ROWS / 128; i++)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p + (long long)i * 128 * ld),
                                       (__attribute__((address_space(3))) void*)(dst + i * 8192), 16, 0, 0);
  } else if (ROWS == 256) {  // [32 k-rows][256 cols], 512-byte rows: piece = 2 k-rows; k-row (tid >> 5) + 16 i, slot tid & 31
    const int krow = tid >> 5, slot = tid & 31;
    const int chunk = ((((slot >> 1) ^ fk(krow))) << 1) | (slot & 1);
    const bf16raw* p = X + (k0 + krow) * ld + tile0 + chunk * 8;
#pragma unroll
    for (int i = 0; i < 2; i++)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p + (long long)i * 16 * ld),
                                       (__attribute__((address_space(3))) void*)(dst + i * 8192), 16, 0, 0);
  } else {  // [32 k-rows][128 cols], 256-byte rows: piece = 4 k-rows; k-row tid >> 4, slot tid & 15
    const int krow = tid >> 4, slot = tid & 15;
    const int chunk = ((((slot >> 1) ^ fk(krow))) << 1) | (slot & 1);
    const bf16raw* p = X + (k0 + krow) * ld + tile0 + chunk * 8;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p),
                                     (__attribute__((address_space(3))) void*)(dst), 16, 0, 0);
  }
}

template <bool TA, bool TB, bool OUTF32>
__global__ __launch_bounds__(512, 4) void gemm_bf16_r256(GemmP p, int ks_xcd) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = (int)(p.N / R_BN);
  const int nt = (int)(p.M / R_BM) * ntn;
  const int bid = blockIdx.x;
  int id, zslice;
  if (ks_xcd > 0) {  // split-K: one k-slice per XCD, all of its tiles on that XCD's L2 (as gemm_bf16_o128)
    const int xcd = bid & 7, r = bid >> 3;
    if (ks_xcd >= 8) { const int per = ks_xcd >> 3; zslice = xcd * per + (r % per); id = r / per; }
    else { zslice = xcd % ks_xcd; id = r * (8 / ks_xcd) + xcd / ks_xcd; }
  } else {
    const int q = nt >> 3, r8 = nt & 7, xcd = bid & 7, loc = bid >> 3;
    id = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + loc;
    zslice = blockIdx.z;
  }
  const long long tm0 = (long long)(id / ntn) * R_BM, tn0 = (long long)(id % ntn) * R_BN;
  const int b = blockIdx.y;
  const long long bo = b / p.binner, bi = b % p.binner;
  const bf16raw* A = (const bf16raw*)p.A + bo * p.sAo + bi * p.sAi;
  const bf16raw* B = (const bf16raw*)p.B + bo * p.sBo + bi * p.sBi;
  const long long coff = bo * p.sCo + bi * p.sCi;
  const long long kbeg = (long long)zslice * p.kchunk;
  long long kend = kbeg + p.kchunk;
  if (kend > p.K) kend = p.K;
  const int nk = (int)((kend - kbeg) / R_BK);

  f4v acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (f4v){0.f, 0.f, 0.f, 0.f};

  // Main loop, software-pipelined by one stage with a TWO-slot ring: at barrier t every wave holds the fragments of stage t
  // in registers (read during the previous iteration), so the slot of stage t can be refilled (DMA of stage t + 2) and the
  // 16 MFMAs of stage t start at once; the fragments of stage t + 1 (landed: waited for before the barrier) are read
  // between them, each register set as soon as its last MFMA has issued.  In the plain form (barrier, 8 fragment reads,
  // 16 MFMAs) all waves left the barrier together into the LDS-read phase and the MFMA pipe waited.
  // A ring of R_ASLOTS slots, B ring of two: at barrier t the workgroup issues B(t + 2) and then A(t + R_ASLOTS); the wait
  // before barrier t leaves the newest A stages (2 DMA instructions each) in flight.
  unsigned char* const abase = smem;
  unsigned char* const bbase = smem + R_ASLOTS * R_ABYTES;
  bf8v fa[4], fb[4];
  if (nk > 0) {
    rstage_glds<TA, 256>(A, p.lda, tm0, kbeg, abase, tid);
    rstage_glds<TB, 128>(B, p.ldb, tn0, kbeg, bbase, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    if (nk > 1) rstage_glds<TB, 128>(B, p.ldb, tn0, kbeg + R_BK, bbase + R_BBYTES, tid);
#pragma unroll
    for (int a = 1; a < R_ASLOTS; a++)
      if (a < nk) rstage_glds<TA, 256>(A, p.lda, tm0, kbeg + (long long)a * R_BK, abase + a * R_ABYTES, tid);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      fa[i] = TA ? rfrag_kmajor<256>(abase, wm * 64 + i * 16, lane) : rfrag_rowmajor(abase, wm * 64 + i * 16, lane);
      fb[i] = TB ? rfrag_kmajor<128>(bbase, wn * 64 + i * 16, lane) : rfrag_rowmajor(bbase, wn * 64 + i * 16, lane);
    }
  }
  int a0 = 0;  // A slot of stage t
  for (int t = 0; t < nk; t++) {
    // own DMA of stage t + 1 has landed; the NEWEST A stage (t + R_ASLOTS - 1: two DMA instructions, issued after
    // B(t + 1)) may still fly
    if (R_ASLOTS >= 3 && t + R_ASLOTS - 1 < nk) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();                                    // everyone's; every wave holds stage t in registers
    if (t + 2 < nk) rstage_glds<TB, 128>(B, p.ldb, tn0, kbeg + (long long)(t + 2) * R_BK, bbase + (t & 1) * R_BBYTES, tid);
    if (t + R_ASLOTS < nk) rstage_glds<TA, 256>(A, p.lda, tm0, kbeg + (long long)(t + R_ASLOTS) * R_BK, abase + a0 * R_ABYTES, tid);
    a0 = a0 + 1 == R_ASLOTS ? 0 : a0 + 1;
    const unsigned char* nsa = abase + a0 * R_ABYTES;               // stage t + 1 (stale data after the last stage: unused)
    const unsigned char* nsb = bbase + ((t + 1) & 1) * R_BBYTES;
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        if (i == 3) {
          fb[j] = TB ? rfrag_kmajor<128>(nsb, wn * 64 + j * 16, lane) : rfrag_rowmajor(nsb, wn * 64 + j * 16, lane);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, TB ? 2 : 1, 0);
        }
      }
      fa[i] = TA ? rfrag_kmajor<256>(nsa, wm * 64 + i * 16, lane) : rfrag_rowmajor(nsa, wm * 64 + i * 16, lane);
      if (i < 3) __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, TA ? 2 : 1, 0);
    }
  }

  // ---- epilogue: f32 accumulators -> LDS in two 64-row halves -> whole 256-byte row segments to HBM (16-byte lanes).
  // In-step A/B showed that full-line coalesced stores (and 16-byte residual / gate loads) matter more than the
  // direct 8-byte-per-lane epilogue's lower instruction count.
  const int c8 = (tid & 15) * 8;
  float bias[8];
  const bool colsum = p.flags & PERO_GEMM_COLSUM;  // p.bias is then an OUTPUT (column sums of the stored result)
  const bool rowdot = p.flags & PERO_GEMM_ROWDOT;  // p.bias is an OUTPUT [M][N/128], p.gate the matrix the rows are dotted with
#pragma unroll
  for (int e = 0; e < 8; e++) bias[e] = (p.bias && !colsum && !rowdot) ? p.bias[tn0 + c8 + e] : 0.f;
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int half = 0; half < 4; half++) {
    __syncthreads();  // main-loop reads (half 0) / previous half's staging reads (half 1) are done
    if (wm == half) {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
          *(f4v*)(smem + (i * 16 + (lane & 15)) * R_EPI_PITCH + (wn * 64 + j * 16 + (lane >> 4) * 4) * 4) = acc[i][j];
    }
    __syncthreads();
    if (OUTF32 && (p.flags & PERO_GEMM_ATOMIC)) {
      // split-K partial sums: one wave instruction adds 64 consecutive floats of a row (256 contiguous bytes)
#pragma unroll
      for (int rr = 0; rr < 8; rr++) {
        const int row = wave * 8 + rr;
        float* C = (float*)p.C + coff + (tm0 + half * 64 + row) * p.ldc + tn0;
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int col = e * 64 + lane;
          atomicAdd(C + col, *(const float*)(smem + row * R_EPI_PITCH + col * 4) * p.alpha);
        }
      }
      continue;
    }
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
      const int row = (tid >> 4) + 32 * rr;
      const f4v v0 = *(const f4v*)(smem + row * R_EPI_PITCH + c8 * 4);
      const f4v v1 = *(const f4v*)(smem + row * R_EPI_PITCH + c8 * 4 + 16);
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
      for (int e = 0; e < 8; e++) v[e] = v[e] * p.alpha + bias[e];
      const long long grow = tm0 + half * 64 + row;
      if (p.resid) {
        const uint4 rr4 = *(const uint4*)((const bf16raw*)p.resid + coff + grow * p.ldr + tn0 + c8);
        const unsigned w[4] = {rr4.x, rr4.y, rr4.z, rr4.w};
#pragma unroll
        for (int e = 0; e < 4; e++) { v[2 * e] += __uint_as_float(w[e] << 16); v[2 * e + 1] += __uint_as_float(w[e] & 0xffff0000u); }
      }
      if (p.flags & PERO_GEMM_RELU) {
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = fmaxf(v[e], 0.f);
      }
      if (rowdot) {
        // this thread's 8 columns of row `grow` (rounded to bf16 as they are stored) times the same columns of p.gate; the 16
        // lanes that share the row (tid & 15 = column group, 128 columns = one block) meet by shuffles
        const uint4 gg = *(const uint4*)((const bf16raw*)p.gate + coff + grow * p.ldg + tn0 + c8);
        const unsigned w[4] = {gg.x, gg.y, gg.z, gg.w};
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          dot += bf2f(f2bf(v[2 * e])) * __uint_as_float(w[e] << 16);
          dot += bf2f(f2bf(v[2 * e + 1])) * __uint_as_float(w[e] & 0xffff0000u);
        }
        dot += __shfl_xor(dot, 1, 64); dot += __shfl_xor(dot, 2, 64); dot += __shfl_xor(dot, 4, 64); dot += __shfl_xor(dot, 8, 64);
        if ((tid & 15) == 0) ((float*)p.bias)[grow * (p.N >> 7) + (tn0 >> 7)] = dot;
      } else if (p.gate && (p.flags & PERO_GEMM_RELU_BITS)) {
        // the ReLU gate as bits: one byte per thread (its 8 columns) and row
        unsigned char* gb = (p.flags & PERO_GEMM_MASK_TILED) ? (unsigned char*)p.gate + ((tn0 + c8) >> 8) * p.M * 32 + grow * 32 + (((tn0 + c8) & 255) >> 3)
                                                             : (unsigned char*)p.gate + grow * p.ldg + ((tn0 + c8) >> 3);
        if (p.flags & PERO_GEMM_RELU) {
          unsigned m = 0;
#pragma unroll
          for (int e = 0; e < 8; e++) m |= (bf2f(f2bf(v[e])) > 0.f ? 1u : 0u) << e;
          *gb = (unsigned char)m;
        } else {
          const unsigned m = *gb;
#pragma unroll
          for (int e = 0; e < 8; e++)
            if (!((m >> e) & 1)) v[e] = 0.f;
        }
      } else if (p.gate) {
        const uint4 gg = *(const uint4*)((const bf16raw*)p.gate + coff + grow * p.ldg + tn0 + c8);
        const unsigned w[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          if (!(__uint_as_float(w[e] << 16) > 0.f)) v[2 * e] = 0.f;
          if (!(__uint_as_float(w[e] & 0xffff0000u) > 0.f)) v[2 * e + 1] = 0.f;
        }
      }
      if (colsum) {
#pragma unroll
        for (int e = 0; e < 8; e++) cs[e] += v[e];
      }
      if (OUTF32) {
        float* C = (float*)p.C + coff + grow * p.ldc + tn0 + c8;
        if (p.flags & PERO_GEMM_ATOMIC) {
#pragma unroll
          for (int e = 0; e < 8; e++) atomicAdd(C + e, v[e]);
        } else {
          if (p.flags & PERO_GEMM_ACCUM) {
            const f4v o0 = *(const f4v*)C, o1 = *(const f4v*)(C + 4);
#pragma unroll
            for (int e = 0; e < 4; e++) { v[e] += o0[e]; v[4 + e] += o1[e]; }
          }
          *(f4v*)C = (f4v){v[0], v[1], v[2], v[3]};
          *(f4v*)(C + 4) = (f4v){v[4], v[5], v[6], v[7]};
        }
      } else {
        uint4 o;
        o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]); o.z = pack2bf(v[4], v[5]); o.w = pack2bf(v[6], v[7]);
        *(uint4*)((bf16raw*)p.C + coff + grow * p.ldc + tn0 + c8) = o;
      }
    }
  }
  if (colsum) {
    // tile column sums: registers (8 rows per thread) -> lanes sharing a column group (xor 16, 32) -> LDS over the 8 waves
    // -> one atomic per column and tile
#pragma unroll
    for (int e = 0; e < 8; e++) { cs[e] += __shfl_xor(cs[e], 16, 64); cs[e] += __shfl_xor(cs[e], 32, 64); }
    __syncthreads();
    float* red = (float*)smem;
    if (lane < 16) {
#pragma unroll
      for (int e = 0; e < 8; e++) red[wave * 128 + lane * 8 + e] = cs[e];
    }
    __syncthreads();
    if (tid < 128) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < 8; w++) t += red[w * 128 + tid];
      atomicAdd((float*)p.bias + tn0 + tid, t);
    }
  }
}

bool pero_gemm_r256_takes(const GemmP& p) { return p.M % R_BM == 0 && p.N % R_BN == 0 && p.K % R_BK == 0; }
void pero_gemm_r256_launch(const GemmP& p, long long batch, int k_split, bool out_f32, hipStream_t st) {
  const bool ta = p.flags & PERO_GEMM_TRANS_A, tb = p.flags & PERO_GEMM_TRANS_B;
  const long long tiles = (p.M / R_BM) * (p.N / R_BN);
  dim3 grid((unsigned)tiles, (unsigned)batch, (unsigned)k_split), block(512);
  int ks_xcd = 0;
  if (batch == 1 && k_split > 1 && pero_xcd_slices(tiles, k_split)) {
    ks_xcd = k_split;
    grid = dim3((unsigned)(tiles * k_split), 1, 1);
  }
#define LAUNCH_R(TA_, TB_, OF_)                                                                                            \
  do {                                                                                                                     \
    PERO_LDS_ATTR((gemm_bf16_r256<TA_, TB_, OF_>), R_LDS_BYTES);                                                           \
    hipLaunchKernelGGL((gemm_bf16_r256<TA_, TB_, OF_>), grid, block, R_LDS_BYTES, st, p, ks_xcd);                          \
  } while (0)
  PERO_LAYOUT_LADDER(LAUNCH_R, ta, tb, out_f32);
#undef LAUNCH_R
}
