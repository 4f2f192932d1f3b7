// Host-side dispatch data of the shape-specialised conv / wgrad kernels (conv_fast_impl.h), shared by
// cnn_conv_fast.hip and cnn_conv_fast_ext.hip: a descriptor per kernel instantiation (built by ONE function
// template from the template arguments, so its numbers and its kernel address cannot disagree), the row types
// of the two shape tables and the switches. Selection and launch (select_conv / select_wgrad) are in
// cnn_conv_fast.hip; cnn_conv_fast_ext.hip only contributes rows.
#pragma once
#include <initializer_list>
#include <vector>

#include "conv_fast_impl.h"

// ---------------------------------------------------------------------------
// switches (tests compare variants through the gt_*_set_* entry points of cnn_conv_fast.hip)
// ---------------------------------------------------------------------------
struct FastSwitches {
  int s2in_ct1 = 1;      // one co tile per wave for the S=(3,5) s2 input-conv dgrad (gt_conv_set_s2in_ct1)
  int regepi = 1;        // fp32 register-direct epilogue of the tile kernel (gt_conv_set_regepi)
  int smallq = 1;        // shorter tiles for small launches (gt_conv_set_smallq) ...
  long smallq_wg = 300;  // ... while the grid is below this many workgroups
  int wgrad_nb = 0;      // 0: per-shape default, 1 / 2: force band buffers (gt_wgrad_set_nb)
  int wgrad_nz = 0;      // 0: automatic column slices, 1 / 2 / 4 / 8 forced (gt_wgrad_set_nz)
};
extern FastSwitches g_fast;   // cnn_conv_fast.hip

// ---------------------------------------------------------------------------
// conv: descriptor, variants, rows
// ---------------------------------------------------------------------------
// one conv_fast_kernel instantiation
struct ConvKernel {
  int KH, KW, NCBI, W, TH, NT, NCO, NWV, PREC, PK, RE, CTX, SCH;
  int lds_fwd, lds_bwd;   // FastCfg::lds of forward (epi_bf16) and other launches
  int TWO;                // two-pass patch staging (conv_fast_impl.h)
  const void* fn;
};

template <int KH, int KW, int NCBI, int W, int TH, int NT, int NCO, int NWV, int PREC, int PK = 0, int RE = 0,
          int CTX = 0, int SCH = 0, int TWO = 0>
static ConvKernel conv_kernel() {
  static_assert((NCO * 8 + 15) / 16 == NT, "NT co tiles of 16 cover the NCO chunks of 8 channels");
  using Cfg = FastCfg<KH, KW, NCBI, W, TH, NT, NCO, PREC, TWO>;
  return {KH, KW, NCBI, W, TH, NT, NCO, NWV, PREC, PK, RE, CTX, SCH, (int)Cfg::lds(true), (int)Cfg::lds(false), TWO,
          reinterpret_cast<const void*>(&conv_fast_kernel<KH, KW, NCBI, W, TH, NT, NCO, NWV, PREC, PK, RE, CTX, SCH, TWO>)};
}

// conditions of a variant (all must hold)
enum : int {
  IF_TH = 1,     // the small-launch rule (smallq_th) returns this variant's tile rows
  IF_PK = 2,     // the packed last co tile applies (pk_ok)
  IF_RE = 4,     // register-epilogue switch on
  IF_S2CT1 = 8,  // s2in_ct1 switch on
  IF_TWO = 16,   // the launch asks for two-pass patch staging (ConvArgs::twopass)
};

struct ConvVariant {
  int cond;
  ConvKernel k;
};
typedef std::vector<ConvVariant> ConvVariants;

// the tile kernel (a wave owns CT <= 2 co tiles x PG pixel groups). fp32 images 16 / 32 wide: its
// register-epilogue twin first, taken while that switch is on. (A plain `if`: the twin is compiled for the
// other shapes too, never run, exactly as the launch macros did -- the set of kernels in the library is unchanged.)
template <int KH, int KW, int NCBI, int W, int TH, int NT, int NCO, int NWV, int PREC, int PK = 0>
static ConvVariants tile(int cond = 0) {
  ConvVariants v;
  if (PREC == 1 && W % 16 == 0) v.push_back({cond | IF_RE, conv_kernel<KH, KW, NCBI, W, TH, NT, NCO, NWV, PREC, PK, 1>()});
  v.push_back({cond, conv_kernel<KH, KW, NCBI, W, TH, NT, NCO, NWV, PREC, PK, 0>()});
  return v;
}

// one co tile per wave (CTX 1), fp32, register-direct epilogue
template <int KH, int KW, int NCBI, int W, int TH, int NT, int NCO, int NWV, int SCH = 1, int TWO = 0>
static ConvVariants ct1(int cond = 0) {
  return {{cond, conv_kernel<KH, KW, NCBI, W, TH, NT, NCO, NWV, 1, 0, 1, 1, SCH, TWO>()}};
}

// One geometry (KH, KW, Cinp / 8, W, Coutp / 8, prec: those of its kernels) with H % hmod == 0. The first
// variant whose conditions hold runs. The small-launch rule halves the tile from hmod rows down to thmin
// (thmin == hmod: none).
struct ConvRow {
  int hmod, thmin;
  ConvVariants v;
  ConvRow(int hmod_, int thmin_, std::initializer_list<ConvVariants> parts) : hmod(hmod_), thmin(thmin_) {
    for (const ConvVariants& p : parts) v.insert(v.end(), p.begin(), p.end());
  }
};

// ---------------------------------------------------------------------------
// wgrad: descriptor and rows
// ---------------------------------------------------------------------------
// one wgrad_fast_kernel (PREC 0) / wgrad_fast_f32_kernel (PREC 1) instantiation
struct WgradKernel {
  int KH, KW, NCBI, NCBO, W, R, NW, NB, PK, NZ, PREC;
  const void* fn;
};

template <int KH, int KW, int NCBI, int NCBO, int W, int R, int NW, int NB, int PK = 0, int NZ = 1>
static WgradKernel wgrad_kernel_f32() {
  return {KH, KW, NCBI, NCBO, W, R, NW, NB, PK, NZ, 1,
          reinterpret_cast<const void*>(&wgrad_fast_f32_kernel<KH, KW, NCBI, NCBO, W, R, NW, NB, PK, NZ>)};
}
template <int KH, int KW, int NCBI, int NCBO, int W, int R, int NW, int NB>
static WgradKernel wgrad_kernel_bf16() {
  return {KH, KW, NCBI, NCBO, W, R, NW, NB, 0, 1, 0,
          reinterpret_cast<const void*>(&wgrad_fast_kernel<KH, KW, NCBI, NCBO, W, R, NW, NB>)};
}

// One geometry (KH, KW, Cinp / 8, Coutp / 8, W, prec) with H % R == 0 and whole bands of R rows per split
// (pps % (R * W) == 0). select_wgrad works out (NW, NB, PK, NZ) from the row and the switches and runs the
// kernel of `k` that has them.
struct WgradRow {
  int KH, KW, NCBI, NCBO, W, R, NW, PREC;
  int NB;   // band buffers unless forced (gt_wgrad_set_nb)
  int NZ;   // column slices per (split, group); 0: automatic (wgrad_nz: NZ 2 keeps NB, NZ 4 has one band
            // buffer, NZ 8 one buffer and 4-wave workgroups)
  std::vector<WgradKernel> k;
};

// fp32, automatic column slices
template <int KH, int KW, int NCBI, int NCBO, int W, int R, int NW, int NB>
static WgradRow wgrad_f32() {
  return {KH, KW, NCBI, NCBO, W, R, NW, 1, NB, 0,
          {wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, 1, 0>(), wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, 1, 1>(),
           wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, 2, 0>(), wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, 2, 1>(),
           wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, NB, 0, 2>(), wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, NB, 1, 2>(),
           wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, 1, 0, 4>(), wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, 1, 1, 4>(),
           wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, 4, 1, 0, 8>(), wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, 4, 1, 1, 8>()}};
}
// fp32 wide layers: NZ column slices per (split, group), single band buffer
template <int KH, int KW, int NCBI, int NCBO, int W, int R, int NW, int NZ>
static WgradRow wgrad_f32z() {
  return {KH, KW, NCBI, NCBO, W, R, NW, 1, 1, NZ,
          {wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, 1, 0, NZ>(), wgrad_kernel_f32<KH, KW, NCBI, NCBO, W, R, NW, 1, 1, NZ>()}};
}
template <int KH, int KW, int NCBI, int NCBO, int W, int R, int NW, int NB>
static WgradRow wgrad_bf16() {
  return {KH, KW, NCBI, NCBO, W, R, NW, 0, NB, 1,
          {wgrad_kernel_bf16<KH, KW, NCBI, NCBO, W, R, NW, 1>(), wgrad_kernel_bf16<KH, KW, NCBI, NCBO, W, R, NW, 2>()}};
}

// rows of user-chosen architectures (cnn_conv_fast_ext.hip), walked after the search-space rows
const std::vector<ConvRow>& conv_rows_ext();
const std::vector<WgradRow>& wgrad_rows_ext();
