// The regime-B plan (free embeddings): what only the psi2 kernels of psi2.hip, psi2_tile.hip and psi2_generic.hip use, and which of them run.  Built
// aside by the first regime-B gp_phase1 and published in gp_ctx::bplan when complete; its two lazy groups likewise by the first phase that needs them.
#pragma once
#include "gp_common.h"

namespace gp {

// kernel families, chosen once per plan (choose_b_path, psi2.hip)
enum class BP1 { PAIRS, PAIRS_MFMA, GENERIC };       // phase 1: psi2_pairs_kernel, psi2_pairs_mfma_kernel, psi2_generic.hip
enum class BP2 { COLS, SYM, TILES, GENERIC };        // phase 2: psi2_cols_kernel, psi2_sym_kernel, psi2_tile_kernel, psi2_generic.hip

// tile-pair phase 2 (psi2_tile.hip): the per-launch buffers
struct BTiles {
  DevBuf<double> ppt;         // [tiles][3Q+1][ch] per-point sums of every tile for the points of one launch
  DevBuf<double> Gt;          // [S][tiles][2][64][Q] grad_Z partials per workgroup
  long ch = 0; int S = 0;     // points and point slices per launch
};

// beyond the compiled latent widths (psi2_generic.hip, Q >= 64)
struct BGeneric {
  DevBuf<double> T, rt;       // [P][M][M] psi2_n of a chunk of points, [P][M][Q + 1] its row contractions
  long P = 0;                 // points per chunk
};

struct BPlan {
  BP1 p1 = BP1::PAIRS;
  BP2 p2 = BP2::COLS;
  int QB = 0;                 // latent table width: the smallest instantiated width >= Q (Q itself on the generic path)
  DevBuf<double> LE;          // [Np][Mp]  1/2 ln c2_n - 1/2 sum_q w_nq (mu_nq - z_mq)^2   (layout: le_interleaved)
  DevBuf<double> LET;         // [Np][Mp]  LEA = LE + sum_q V_nq z_mq^2 (n-major)
  DevBuf<double> Vn;          // [Np][Q]   -1/4 (alpha_q - w_nq)
  DevBuf<double> Wn;          // [Np][Q]   w_nq = alpha_q / (2 alpha_q S_nq + 1)
  DevBuf<double> V2P, WP, MUP;    // [Np][QB]  -2 V_nq, w_nq, mu_nq, zero-padded to QB
  DevBuf<double> alphaP;      // [QB]      alpha, zero-padded
  DevBuf<double> ZP, Z1P;     // [Mp][QB]  Z zero-padded (rows >= M and columns >= Q are zero); the same with a column of ones at index Q (QB > Q)
  DevBuf<double> Z1S;         // [Mp][RT]  [Z | 1 at index QB | 0], RT = QB + 1 rounded up to 4: B operand of psi2_sym_kernel's row-side MFMAs (SYM only)
  DevBuf<double> lnc2h;       // [Np]      1/2 ln c2_n
  DevBuf<double> Bbar4;       // [Mp][Mp]  Bbar with four ROWS interleaved, element (m, m') at ((m / 4) Mp + m') 4 + m % 4 (bbar_interleave_kernel)
  DevBuf<double> pp;          // [groups][3QB+1][Np] per-point running sums sr, zr, z2r, zt of phase 2
  DevBuf<double> Gpart, Gtmp, gapart2;    // [pb_blocks][M][Q] per-workgroup and [64][M][Q] second-level grad_Z partials, [pb_blocks][Q] grad_alpha's
  DevBuf<double> DZ2;         // [M][M][Q] (z_mq - z_m'q)^2: the compat path's per-point psi2 tensor only (b_point_tables, allocated on first use)
  DevBuf<int> ptiles;         // upper-triangular 16x16 tile table of psi2_pairs_kernel
  DevBuf<int> tiles64;        // upper-triangular 64x64 tile table of psi2_pairs_mfma_kernel and the tile-pair phase 2
  DevBuf<int> sym_sched;      // [rounds][waves] tile of every wave of psi2_sym_kernel in every round (I | J << 16, -1 idle; SYM only)
  int n_ptiles = 0, n_tiles64 = 0;
  size_t part_need = 0;       // doubles of the shared workspace the pair kernels' split-n partials take (reserved when the plan is built)
  int nslab = 0, ppb = 0, pb_blocks = 0;     // phase 2: 64-column slabs of M, points per workgroup, workgroups along the points
  int sym_nw = 0, sym_rounds = 0;
  std::unique_ptr<BTiles> tiles;      // TILES: built by the first tile-pair phase 2
  std::unique_ptr<BGeneric> gen;      // GENERIC: built by the first phase that needs it
  // what poison mode (gp_set_globals) refills with NaN bytes at every evaluation: written by each evaluation before it is read
  std::vector<const DevBuf<double>*> poisoned() const {
    std::vector<const DevBuf<double>*> v = {&LE, &LET, &Gpart, &gapart2, &Gtmp, &pp};
    if (tiles) { v.push_back(&tiles->ppt); v.push_back(&tiles->Gt); }
    return v;
  }
};

// the points' finish of phase 2 (psi2_tile.hip) for the points n0 <= n < n1: row i of group g of the summed sums [sr | zr_q | z2r_q | zt_q] of point n sits at
// pp[g GS + i CH + n - n0], the rows of one kind QK apart; ngrp groups are added in order
struct PT2Fin {
  const double* pp; const double* Wn; const double* mu; const double* S; const double* alpha;
  double* gmu; double* gS; double* gapart2; long n0, n1, CH, GS; int Q, QK, ngrp, accumulate;
};
int launch_points_finish(gp_ctx* c, int blocks, const PT2Fin& f);

// shared by the psi2 trio
int run_le_generic(gp_ctx* c);
int run_phase1_b_generic(gp_ctx* c);
int run_phase2_b_generic(gp_ctx* c);
int run_phase2_b_tiles(gp_ctx* c);

}  // namespace gp
