// FP64 matrix-core building blocks for gfx950 (MI355X).
//
// Measured on MI355X (tools/ubench, profiles/ubench_f64.txt):
//   v_mfma_f64_16x16x4_f64      ~36 TF  (128+ cycles / instruction: HALF the FP64 rate)
//   v_mfma_f64_4x4x4_4b_f64     ~74 TF  (16 cycles / instruction, = the FP64 VALU FMA rate, same pipe)
//   v_fma_f64 (VALU)            ~74 TF
// so the dense FP64 contractions use the 4x4x4 (4-block) MFMA: full rate with 1/4 of the issue slots and
// 1/4 of the operand traffic of VALU FMAs.
//
// Lane map of __builtin_amdgcn_mfma_f64_4x4x4f64 (verified by tools/ubench/f64_ubench2.hip): lane l belongs to
// block b = (l>>2)&3;  A operand: A_b[i = l&3][k = l>>4];  B operand: B_b[k = l>>4][j = l&3];
// result: D_b[i = l>>4][j = l&3].  We give the four blocks four consecutive row-quads and the SAME 4 columns,
// so one instruction is a 16x4 (rows x cols) output tile with k = 4:
//   A register: lane l holds A[row = l&15][k = l>>4]                     (64 distinct values)
//   B register: lane l holds B[k = l>>4][col = l&3]                      (16 distinct values, replicated over (l>>2)&3)
//   D register: lane l holds D[row = 4*((l>>2)&3) + (l>>4)][col = l&3]
// A wave owns a 64x64 output tile: 4 A registers x 16 B registers = 64 accumulators (128 VGPRs).
#pragma once
#include <hip/hip_runtime.h>

namespace gp {

// compile-time loop: f(IC<B>{}), ..., f(IC<E-1>{}) -- the index is a constant expression inside f (immediate offsets, register arrays)
template <int I> struct IC { static constexpr int value = I; };
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) { f(IC<B>{}); static_for<B + 1, E>(f); }
}

constexpr int TILE = 128;          // workgroup output tile (rows and cols), 4 waves as 2x2 of 64x64
constexpr int WT = 64;             // wave tile
constexpr int KC = 16;             // k-chunk staged through LDS per iteration
constexpr int LDS_RC = TILE + 16;  // LDS row stride (doubles) of a [KC][TILE] tile (operand contiguous along its free index):
                                   // +16 doubles puts the two k-rows a 32-lane read group touches on different bank halves
                                   // (unpadded, every one of the 20 operand reads per k-step is a 2-way conflict)
constexpr int TILE_LDS_DOUBLES = KC * LDS_RC;  // 2304 doubles = 18 KB per operand tile (a [TILE][KC] tile uses 2048 of them)

// how an operand tile is stored (in global memory and, identically, in LDS)
enum Layout : int {
  FREE_CONTIG = 0,   // stored [k][r]: rows indexed by k, free index r contiguous
  K_CONTIG = 1       // stored [r][k]: rows indexed by r, k contiguous
};

// Inline asm keeps the accumulation in place (dst == srcC): with the builtin hipcc renames accumulators to make
// room for ds_read2 destinations and then pays ~130 v_mov_b64 per k-chunk to rotate them back.  The operands
// come straight from ds_read (the compiler's s_waitcnt covers them).  hipcc does not model the MFMA inside the
// string, so anything that READS an accumulator with a non-MFMA instruction must first pass mfma_drain().
__device__ __forceinline__ void mfma444_acc(double& c, double a, double b) {
  asm volatile("v_mfma_f64_4x4x4_4b_f64 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// first MFMA of an accumulation: C = 0 as an inline constant (no zeroing moves; "&": the result may not share a register with an operand)
__device__ __forceinline__ void mfma444_zero(double& c, double a, double b) {
  asm volatile("v_mfma_f64_4x4x4_4b_f64 %0, %1, %2, 0" : "=&v"(c) : "v"(a), "v"(b));
}
// wait states between the last in-flight MFMA and a VALU/VMEM read of an accumulator (4-pass DGEMM result).  The s_nop is
// tied to one accumulator only; every OTHER accumulator that is read afterwards must pass acc_fence (an empty asm with the
// register as an in/out operand, placed after the s_nop: volatile asms keep their order), otherwise the scheduler may
// legally hoist such a read to just behind that accumulator's last MFMA -- inside the hazard window.
__device__ __forceinline__ void mfma_drain(double& last_acc) { asm volatile("s_nop 15" : "+v"(last_acc)); }
__device__ __forceinline__ void acc_fence8(double (&x)[8]) {
  asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]));
}
template <int N>
__device__ __forceinline__ void acc_fence(double (&x)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(x[i]));
}
__device__ __forceinline__ double mfma444(double a, double b, double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// ---- LDS operand reads as explicit ds_read_b64 -----------------------------------------------------------------------
// hipcc merges two 8-byte LDS loads off one address register into ds_read2_b64 / ds_read2st64_b64.  Those are serviced in
// 16-lane groups over 32 banks (half the rate of two ds_read_b64, MI355X_MICROARCH.md LDS table), and the K_CONTIG image above --
// laid out for the 32-lane groups of ds_read_b64 -- becomes a 2-way bank conflict on every A-operand read (PMC: 6.2e8 conflict
// cycles in the phase-2 kernel, 0 in phase 1 whose operands are both FREE_CONTIG).  The hot loops therefore issue their reads
// through inline asm; the compiler does not track those, so the loops carry their own s_waitcnt lgkmcnt(n): LDS returns in
// order, and lgkmcnt(n) bounds ALL outstanding LGKM operations, so at most n of the wave's reads are still in flight.
typedef __attribute__((address_space(3))) const char lds_cchar;
__device__ __forceinline__ unsigned lds_byte_addr(const double* p) { return (unsigned)(size_t)(lds_cchar*)p; }
template <int OFF>
__device__ __forceinline__ double ds_read64(unsigned byte_addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read_b64 immediate offset is 16 bits");
  double v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(byte_addr), "n"(OFF) : "memory");
  return v;
}
template <int N>
__device__ __forceinline__ void lgkm_wait() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }

struct Acc {
  double v[4][16];
  // drain the matrix pipe and order every later read of this tile's accumulators behind it
  __device__ __forceinline__ void drain() {
    asm volatile("s_nop 15" : "+v"(v[3][15]));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      asm volatile("" : "+v"(v[i][0]), "+v"(v[i][1]), "+v"(v[i][2]), "+v"(v[i][3]), "+v"(v[i][4]), "+v"(v[i][5]), "+v"(v[i][6]), "+v"(v[i][7]));
      asm volatile("" : "+v"(v[i][8]), "+v"(v[i][9]), "+v"(v[i][10]), "+v"(v[i][11]), "+v"(v[i][12]), "+v"(v[i][13]), "+v"(v[i][14]), "+v"(v[i][15]));
    }
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) v[i][j] = 0.0;
  }
};

// element (row, col) inside the wave's 64x64 tile that accumulator [ar][bc] holds for this lane
__device__ __forceinline__ int acc_row(int ar, int lane) { return 16 * ar + 4 * ((lane >> 2) & 3) + (lane >> 4); }
__device__ __forceinline__ int acc_col(int bc, int lane) { return 4 * bc + (lane & 3); }

// ---- global -> LDS staging of one operand tile by LDS-DMA (global_load_lds_dwordx4), 256 threads ----------------
// The DMA writes wave-uniform base + lane*16 B, so each wave-instruction fills 1 KB of contiguous LDS.
//  FREE_CONTIG tile [KC][TILE]: one instruction = one k-row (128 doubles); rows are padded to LDS_RC doubles
//    (padding sits BETWEEN instructions, which is allowed) so that the two k-rows a 32-lane group reads land on
//    different bank halves.
//  K_CONTIG tile [TILE][KC]: one instruction = 8 rows x 128 B, unpadded.  To read 16 rows x one k conflict-free
//    the image is permuted through the SOURCE address (the destination is fixed by the hardware):
//      slot(row)   = row with bits 0 and 3 swapped          (so the slot parity = bit 3 of the row)
//      pairpos(kp) = kp ^ (row & 7)                         (16-byte pair index inside the 128-B row)
//    A 32-lane read group (16 rows, k and k+1) then covers all 32 8-byte bank positions exactly once.
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

__device__ __forceinline__ void glds16(const double* gsrc, double* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void*)gsrc, (lds_void*)lds_wave_base, 16, 0, 0);
}
__device__ __forceinline__ int swap03(int r) { return (r & ~9) | ((r & 1) << 3) | ((r >> 3) & 1); }

// index (in doubles) of element (r, k) inside a K_CONTIG LDS tile
__device__ __forceinline__ int kc_index(int r, int k) { return swap03(r) * KC + 2 * ((k >> 1) ^ (r & 7)) + (k & 1); }

// src -> element (k0, r0) [FREE_CONTIG] or (r0, k0) [K_CONTIG]; ld = row stride in doubles (even, 16-B aligned rows)
template <Layout L>
__device__ __forceinline__ void tile_dma(double* lds_tile, const double* __restrict__ src, long ld, int wave, int lane) {
  if (L == FREE_CONTIG) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wave * 4 + i;
      glds16(src + (long)row * ld + 2 * lane, lds_tile + row * LDS_RC);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int slot = (wave * 4 + i) * 8 + (lane >> 3);
      const int row = swap03(slot);
      const int kp = (lane & 7) ^ (row & 7);
      glds16(src + (long)row * ld + 2 * kp, lds_tile + (wave * 4 + i) * 8 * KC);
    }
  }
}

// all of this wave's DMAs have landed
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---- one KC-deep update of the wave's 64x64 accumulator from LDS tiles ---------------------------------------
// Per-lane LDS offsets (in doubles) are split into a lane-dependent base, computed once per kernel, plus
// compile-time constants that fold into the ds_read immediate offset.
//   FREE_CONTIG:  idx(k, x) = k*LDS_RC + x                                   base = lk*LDS_RC + x_lane
//   K_CONTIG A :  row = wrow0 + 16*ar + lr; idx = kc_index(row, 4*k4 + lk)   base[k4] (4 values) + 256*ar
//   K_CONTIG B :  col = wcol0 + 4*bc + lj;  idx = kc_index(col, 4*k4 + lk)   base[k4 & 1] (2 values) + const(bc, k4)
struct LaneOfs {
  int a[4];  // A operand base per k4 (FREE_CONTIG uses a[0] only)
  int b[2];  // B operand base per k4 parity (FREE_CONTIG uses b[0] only)
};

template <Layout LA, Layout LB>
__device__ __forceinline__ LaneOfs lane_offsets(int wrow0, int wcol0, int lane) {
  const int lr = lane & 15, lk = lane >> 4, lj = lane & 3;
  LaneOfs o;
  if (LA == FREE_CONTIG) {
    o.a[0] = o.a[1] = o.a[2] = o.a[3] = lk * LDS_RC + wrow0 + lr;
  } else {
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4)
      o.a[k4] = (wrow0 + swap03(lr)) * KC + 2 * (((k4 ^ ((lr >> 1) & 3)) << 1) | ((lk >> 1) ^ (lr & 1))) + (lk & 1);
  }
  if (LB == FREE_CONTIG) {
    o.b[0] = o.b[1] = lk * LDS_RC + wcol0 + lj;
  } else {
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      const int P = ((par ^ ((lj >> 1) & 1)) << 1) | ((lk >> 1) ^ (lj & 1));
      o.b[par] = wcol0 * KC + (lj & 1) * 128 + (lj & 2) * 16 + 2 * P + (lk & 1);
    }
  }
  return o;
}

template <Layout LA, Layout LB>
__device__ __forceinline__ void load_operands(const double* sA, const double* sB, const LaneOfs& o, int k4, double (&a)[4], double (&b)[16]) {
#pragma unroll
  for (int ar = 0; ar < 4; ++ar)
    a[ar] = (LA == FREE_CONTIG) ? sA[o.a[0] + 4 * k4 * LDS_RC + 16 * ar] : sA[o.a[k4] + 256 * ar];
#pragma unroll
  for (int bc = 0; bc < 16; ++bc)
    b[bc] = (LB == FREE_CONTIG)
                ? sB[o.b[0] + 4 * k4 * LDS_RC + 4 * bc]
                : sB[o.b[k4 & 1] + (bc & 1) * 64 + ((bc >> 1) & 1) * 16 + (bc >> 2) * 256 + (((k4 >> 1) ^ (bc & 1)) << 3)];
}

__device__ __forceinline__ void mma_step(Acc& acc, const double (&a)[4], const double (&b)[16]) {
#pragma unroll
  for (int ar = 0; ar < 4; ++ar)
#pragma unroll
    for (int bc = 0; bc < 16; ++bc) mfma444_acc(acc.v[ar][bc], a[ar], b[bc]);
}

// the first k-step of a chain: C is the inline constant 0, the accumulators need no zeroing in C++ (DESIGN.md section 3's rule)
__device__ __forceinline__ void mma_step_zero(Acc& acc, const double (&a)[4], const double (&b)[16]) {
#pragma unroll
  for (int ar = 0; ar < 4; ++ar)
#pragma unroll
    for (int bc = 0; bc < 16; ++bc) mfma444_zero(acc.v[ar][bc], a[ar], b[bc]);
}

// Operand registers are double-buffered: the ds_reads of step k4+1 are issued before the 64 MFMAs of step k4,
// so one wave alone keeps the matrix pipe busy inside a chunk.  FIRST: the chunk opens the accumulation (mma_step_zero).
template <Layout LA, Layout LB, bool FIRST = false>
__device__ __forceinline__ void mma_chunk(const double* sA, const double* sB, Acc& acc, const LaneOfs& o) {
  double a0[4], b0[16], a1[4], b1[16];
  load_operands<LA, LB>(sA, sB, o, 0, a0, b0);
  load_operands<LA, LB>(sA, sB, o, 1, a1, b1);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (FIRST) mma_step_zero(acc, a0, b0);
  else mma_step(acc, a0, b0);
  __builtin_amdgcn_sched_barrier(0);
  load_operands<LA, LB>(sA, sB, o, 2, a0, b0);
  __builtin_amdgcn_sched_barrier(0);
  mma_step(acc, a1, b1);
  __builtin_amdgcn_sched_barrier(0);
  load_operands<LA, LB>(sA, sB, o, 3, a1, b1);
  __builtin_amdgcn_sched_barrier(0);
  mma_step(acc, a0, b0);
  __builtin_amdgcn_sched_barrier(0);
  mma_step(acc, a1, b1);
}

// ---- the eight-wave form -------------------------------------------------------------------------------------
// p1_kernel8, p1v2_kernel's F jobs, p2_fast8_kernel and p2_gen8_kernel (psi.hip, p1v2.hip) run one structure: eight waves on a 128 x 128
// workgroup tile, every 64 x 64 quadrant shared by two waves (64 rows x 32 columns: 32 accumulators per wave, four waves per SIMD), KC-deep
// chunks staged by LDS-DMA into two buffers, operand reads as explicit ds_read_b64 and an lgkmcnt ladder in front of the 32 in-place MFMAs
// of a k-step.  The k-step lives here once; the chunk staging of phase 2 in two forms that must write the same LDS image -- stage8_kf (p2_gen8_kernel,
// p2_rem_kernel) and stage8_kf_s (p2_fast8_kernel): a change to the K_CONTIG swizzle is a change to both.  The loops around them stay in the kernels: they differ in what travels
// during the last chunk, and hipcc's schedule of the surrounding scalar code follows the order of the source statements, so every piece
// below was introduced only where the kernel's assembly stayed the same, instruction for instruction (profiles/kloop8_asm_identity.txt).
// p1_kernel8 takes the k-step only: with Wave8 or stage8_ff its assembly changes.
struct Wave8 {
  int wave, quad, half;   // wave = quad + 4 half: the two waves of a quadrant sit on the same SIMD
  int wr, wc;             // the quadrant's row and column
  int wrow0, wcol0;       // first row and column of the wave's 64 x 32 block inside the workgroup tile
  __device__ __forceinline__ explicit Wave8(int w)
      : wave(w), quad(w & 3), half(w >> 2), wr(quad >> 1), wc(quad & 1), wrow0(wr * WT), wcol0(wc * WT + 32 * half) {}
};

// One k-step (k = 4) of the wave's 64 x 32 block: 4 A + 8 B operand reads, then 32 MFMAs that start as soon as A and the first B have landed
// (twice the LDS rate of the ds_read2_b64 pairs hipcc would form, see above).  aA / aB: LDS byte addresses of the lane's first A / B operand.
//   B, and A when it is FREE_CONTIG: k-step K4 of the chunk is an immediate offset of K4 * 4 rows
//   K_CONTIG A (A_KCONTIG): the caller's aA already carries LaneOfs::a[K4]; the four 16-row groups are 2048 B apart
template <int K4, bool A_KCONTIG>
__device__ __forceinline__ void kstep8(double (&acc)[4][8], unsigned aA, unsigned aB) {
  double a[4], b[8];
  static_for<0, 4>([&](auto ic) {
    constexpr int ar = decltype(ic)::value;
    a[ar] = ds_read64<A_KCONTIG ? 2048 * ar : K4 * 4 * LDS_RC * 8 + 128 * ar>(aA);
  });
  static_for<0, 8>([&](auto jc) { constexpr int j = decltype(jc)::value; b[j] = ds_read64<K4 * 4 * LDS_RC * 8 + 32 * j>(aB); });
  static_for<0, 8>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    lgkm_wait<7 - j>();
#pragma unroll
    for (int ar = 0; ar < 4; ++ar) mfma444_acc(acc[ar][j], a[ar], b[j]);
  });
}

// Chunk staging: 16 LDS-DMA instructions per operand tile, two per wave.
// Both operands FREE_CONTIG with row stride ld (rows of 128 doubles) into the double-buffered pair of tiles lds[buf]
using Tiles8 = double[2][2][TILE_LDS_DOUBLES];
__device__ __forceinline__ void stage8_ff(Tiles8& lds, int buf, const double* a, const double* b, long ld, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * 2 + i;
    glds16(a + (long)row * ld + 2 * lane, lds[buf][0] + row * LDS_RC);
    glds16(b + (long)row * ld + 2 * lane, lds[buf][1] + row * LDS_RC);
  }
}
// A K_CONTIG (row stride lda), B FREE_CONTIG (row stride ldb) into buf = [A tile | B tile]; lane offsets are 32-bit (uniform base + offset addressing)
__device__ __forceinline__ void stage8_kf(double* buf, const double* a, const double* b, long lda, int ldb, int wave, int lane) {
  int ld_ = lane;
  asm volatile("" : "+v"(ld_));                             // recomputed per chunk (a handful of integer ops) instead of held in registers
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int I = wave * 2 + i;
    const int row = swap03(I * 8 + (ld_ >> 3));
    // byte offset as an unsigned 32-bit value: uniform base + 32-bit lane offset addressing (one address register instead of two)
    glds16(reinterpret_cast<const double*>(reinterpret_cast<const char*>(a) + (unsigned)(8 * (row * (int)lda + 2 * ((ld_ & 7) ^ (row & 7))))),
           buf + I * 8 * KC);
    glds16(b + (long)I * ldb + 2u * ld_, buf + TILE_LDS_DOUBLES + I * LDS_RC);
  }
}
// ---- the same chunk with the lane patterns held and the advance in scalar registers ------------------------------------------------
// stage8_kf's lane patterns never change during a launch, only a wave-uniform base moves from chunk to chunk; stage8_kf nevertheless
// rebuilds them in VALU code for every chunk, between the MFMAs (27 VALU instructions per chunk and wave in p2_fast8_kernel<3>, three of
// them 64-bit adds: profiles/stage8_buffer_dma.txt).  Here every LDS-DMA is  wave-uniform 64-bit base (SGPR pair) + 32-bit lane offset:
//   A's lane offset (kf8_lane) is computed once per row tile from an opaque copy of the lane id and held across the tile's k-loop,
//   the wave's rows and the chunk advance go into the scalar base (s_add_u32 / s_addc_u32), so nothing is limited to 32 bits but the
//   lane offset itself: at most 8 * (14 lda + 16) bytes for A, 1008 for B (STAGE8_MAX_LDA; the launch function checks it and reports).
// The LDS image, the bytes moved and the order of the instructions are stage8_kf's.
// (The buffer form, buffer_load_dwordx4 ... offen lds with the tile's window as descriptor, was built first and is the same instruction
// count per chunk, but its two descriptors are eight more SGPRs held across the k-loop of a kernel that already uses 104: seven SGPR
// spills and 8 B of scratch in p2_fast8_kernel<2> and <3>.  See profiles/stage8_buffer_dma.txt.)
constexpr long STAGE8_MAX_LDA = 1L << 24;            // doubles: 8 * (14 lda + 16) < 2^31
// An asm statement, because hipcc, given base + zero-extended offset in C++, widens the held offsets to 64-bit pairs and adds the base with
// v_lshl_add_u64 per instruction (six VGPRs held, scratch spills).  M0 is compiler-reserved: saved and restored inside the statement.  hipcc
// does not count the load: every consumer waits by dma_wait() / an explicit vmcnt as before, and its own vmcnt waits only become stricter.
// (Fragile where an explicit vmcnt(n > 0) follows: a compiler-tracked global load placed between such a DMA and that wait is counted by the
// hardware and not by the n in the source.)  sbase and lds_wave_base go to "s" operands: both must be wave-uniform.
__device__ __forceinline__ void glds16_sv(const double* sbase, unsigned voffset, double* lds_wave_base) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voffset), "s"(sbase), "s"(lds_byte_addr(lds_wave_base)) : "memory");
}
// Lane patterns of stage8_kf as byte offsets.  Instruction i of wave w moves slots (2 w + i) * 8 + (lane >> 3), i.e. rows
//   swap03(slot) = 16 w + r_l + i,   r_l = ((lane >> 3) & 6) | ((lane >> 3) & 1) << 3    (even, lane-only)
// and 16-byte pair (lane & 7) ^ (row & 7) of them.  With x = (lane & 7) ^ (r_l & 7):  i = 0 reads pair x, i = 1 pair x ^ 1, so
//   va = 8 r_l lda + 16 x   and the second instruction's offset is va ^ 16  (8 r_l lda is a multiple of 32: r_l and lda are even);
// the rows 16 w + i go into the scalar base.  B: row 2 w + i in the scalar base, lane offset 16 lane.
__device__ __forceinline__ unsigned kf8_lane(int lane, long lda) {
  const int g = lane >> 3, rl = (g & 6) | ((g & 1) << 3);
  return 8u * ((unsigned)rl * (unsigned)lda) + 16u * (unsigned)((lane & 7) ^ (rl & 7));
}
// a / b: the chunk's first element of the WAVE's first row: row 16 wave of the A row tile / k row 2 wave of the B column tile
__device__ __forceinline__ void stage8_kf_s(double* buf, const double* a, const double* b, long lda, int ldb, int wave, unsigned va_, int lane) {
  unsigned va = va_, vb = (unsigned)lane;
  asm volatile("" : "+v"(va), "+v"(vb));            // va ^ 16 and 16 lane are one VALU instruction each per chunk, not two more held registers
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int I = wave * 2 + i;
    glds16_sv(a + (long)i * lda, va ^ (16u * i), buf + I * 8 * KC);
    glds16_sv(b + (long)i * ldb, 16u * vb, buf + TILE_LDS_DOUBLES + I * LDS_RC);
  }
}
// (Staging the B tile for every second chunk only -- 25 % fewer LDS-DMA instructions per flop, what a 256 x 128 workgroup tile would issue -- and
// no staging at all were measured on p2_fast8_kernel with the same instruction stream otherwise: profiles/r03_p2_dma_ablation.txt, r04_power_ab.txt.)

}  // namespace gp
