// Shape-specialised implicit-GEMM convolution (forward and data-gradient) and weight gradient: the shape
// tables of the search-space shapes (one row per layer geometry), the pure selection on top of them
// (select_conv / select_wgrad: arguments -> instantiation, grid, block, LDS) and the one launch site. The kernel
// templates (and the design notes) are in conv_fast_impl.h, the row types in conv_fast_host.h; the rows of
// user-chosen architectures in cnn_conv_fast_ext.hip are walked after the ones here.
#include "conv_fast_host.h"

// ---------------------------------------------------------------------------
// switches
// ---------------------------------------------------------------------------
FastSwitches g_fast;

// every setter returns the previous value (tests restore with it)
static int swap_switch(int& sw, int v) {
  const int old = sw;
  sw = v;
  return old;
}

// The S=(3,5) s2 input-conv dgrad (5x5, 50 -> 20) with one co tile per wave and 4 pixel groups each
// instead of the packed tile's 2 tiles x 2 groups: 33 % more MFMAs but half the weight loads per MFMA;
// same-box A/B 126 -> 114 us per launch at 25 groups, population step -1.6 % (profiles/conv_s2in_dgrad_ct1_ab_r3.txt).
// Runtime setter (tests only) so both variants are compared against the fp64
// oracle on one launch in one process (tests/test_hip_fp32.py::test_s2in_dgrad_variants): both 1.3e-6 of
// the output range (torch fp32: 7.1e-7), channels 0-15 bitwise equal, deterministic; the 2-rank DP
// trajectory stays within the derived summation-order bound (tests/test_hip_dp.py). On by default since
// round 4 (profiles/conv_s2in_dgrad_ct1_r4.txt).
extern "C" int gt_conv_set_s2in_ct1(int on) { return swap_switch(g_fast.s2in_ct1, on); }

// fp32 register-direct epilogue in the tile kernel (tests compare it with the LDS tile): no LDS output tile,
// no second barrier, the pool from lane shuffles. On by default: 2-19 % faster per fp32 conv launch,
// bit-identical (profiles/conv_f32_regepi_ab_r3.txt)
extern "C" int gt_conv_set_regepi(int on) { return swap_switch(g_fast.regepi, on); }

// Small launches (few groups per launch: the reference's sequential folds, one
// rank's share of a config-3 generation): at 2 groups the 8-row tiles of the
// 16x16 stage make 128 workgroups for 256 CUs. Shorter tiles (4 or 2 rows;
// 2 rows = one co tile per wave, so a wave still holds whole row pairs for the
// fused pool) multiply the grid. Every output's k loop (order of k-steps and
// of the six split terms) is the same for any tile height: results are
// bit-identical to the 8-row tiles (tests/test_hip_kernels.py), so a
// candidate's result still does not depend on how many groups share its
// launch. gt_conv_set_smallq(0) disables (tests compare both).
extern "C" int gt_conv_set_smallq(int on) { return swap_switch(g_fast.smallq, on); }

// tile rows for a launch whose default tile has TH rows: halve while the grid
// is below smallq_wg workgroups (300: about one per CU; at 5 and 10 groups the
// 8-row tiles measured faster than 4-row ones, profiles/conv_tile_threshold_ab_r4.txt), down to THMIN
static int smallq_th(const ConvArgs* a, int TH, int THMIN) {
  if (!g_fast.smallq) return TH;
  int th = TH;
  while (th > THMIN && (long)a->ngroups * a->B * (a->H / th) < g_fast.smallq_wg) th >>= 1;
  return th;
}

// the packed last co tile applies: fp32, the real output channels leave <= 4 in the last 16-channel tile
static bool pk_ok(const ConvArgs* a, int nt) {
  const int last = a->cout_real - 16 * (nt - 1);
  return a->prec == 1 && a->cout_real > 0 && last >= 1 && last <= 4;
}

// ---------------------------------------------------------------------------
// conv shape table: (KH, KW, NCBI, W, TH, NT, NCO, NWV, ...) of each variant; ConvRow(hmod, thmin, variants)
// ---------------------------------------------------------------------------
static const std::vector<ConvRow>& conv_rows() {
  static const std::vector<ConvRow> rows = {
    // --- fp32 ---
    // Genetic-CNN CIFAR-shaped S=(3,5) space, kernels (20, 50), 5x5 stage convs
    // (8-wave workgroups for these fp32 tiles: 35-40 % slower per launch, r5/conv_f32_nwv8_ab_r5.txt)
    {8, 4, {tile<5, 5, 1, 32, 4, 2, 3, 2, 1, 1>(IF_TH | IF_PK), tile<5, 5, 1, 32, 4, 2, 3, 2, 1>(IF_TH),
            tile<5, 5, 1, 32, 8, 2, 3, 4, 1, 1>(IF_PK), tile<5, 5, 1, 32, 8, 2, 3, 4, 1>()}},   // s1 input conv (3 -> 20)
    // s1 nodes / output conv, and their dgrad (20 -> 20)
    {8, 4, {tile<3, 3, 3, 32, 4, 2, 3, 2, 1, 1>(IF_TH | IF_PK), tile<3, 3, 3, 32, 4, 2, 3, 2, 1>(IF_TH),
            tile<3, 3, 3, 32, 8, 2, 3, 4, 1, 1>(IF_PK), tile<3, 3, 3, 32, 8, 2, 3, 4, 1>()}},
    // s2 input conv (20 -> 50): one co tile per wave as well (fwd 84-85 vs 86-90 us, r5/conv_s2n_ct1_ab_r5.txt)
    // (a packed tile here needs every wave to own all 4 co tiles: 2x the weight traffic per MFMA,
    // measured 20 % slower than the 2 + 2 split -- profiles/conv_f32_packed_tile_ab_r2.txt)
    {8, 2, {tile<5, 5, 3, 16, 4, 4, 7, 4, 1>(IF_TH), ct1<5, 5, 3, 16, 2, 4, 7, 4>(IF_TH), ct1<5, 5, 3, 16, 8, 4, 7, 4, 0>()}},
    // s2 nodes / output conv, and their dgrad (50 -> 50): one co tile per wave, all 8 pixel groups (170 VGPRs
    // at 2 waves/SIMD): half the weight-fragment loads per MFMA of the 2 co x 4 group split, -1 % per
    // population step at 25 and 80 groups (r5/conv_s2n_ct1_ab_r5.txt; the enforced-pipeline build spills here).
    // Launches that set ConvArgs::twopass run the 8-row tile with two-pass patch staging (35 KB of LDS instead
    // of 70, 161 VGPRs: 3 workgroups per CU instead of 2; bit-identical, profiles/r7/conv_s2_twopass_r7.txt);
    // the 4- and 2-row small-launch tiles are the same for either setting
    {8, 2, {tile<3, 3, 7, 16, 4, 4, 7, 4, 1>(IF_TH), ct1<3, 3, 7, 16, 2, 4, 7, 4>(IF_TH),
            ct1<3, 3, 7, 16, 8, 4, 7, 4, 0, 1>(IF_TWO), ct1<3, 3, 7, 16, 8, 4, 7, 4, 0>()}},
    // s2 input conv dgrad (50 -> 20): one co tile per wave while s2in_ct1 is on, else the packed tile
    {8, 4, {ct1<5, 5, 7, 16, 4, 2, 3, 4>(IF_S2CT1 | IF_TH), ct1<5, 5, 7, 16, 8, 2, 3, 4>(IF_S2CT1),
            tile<5, 5, 7, 16, 8, 2, 3, 4, 1, 1>(IF_PK), tile<5, 5, 7, 16, 8, 2, 3, 4, 1>()}},
    // deep S=(3,4,5) space, kernels (20, 50, 100): stage 3 at 8x8, one image per workgroup
    // (narrow images, W < 16, and the wide deep-space shapes: tile kernel only)
    {8, 8, {tile<5, 5, 7, 8, 8, 7, 13, 7, 1>()}},    // s3 input conv (50 -> 100): one co tile per wave, 7 waves
    {8, 8, {tile<3, 3, 13, 8, 8, 7, 13, 7, 1>()}},   // s3 nodes / output conv, and their dgrad (100 -> 100)
    {8, 8, {tile<5, 5, 13, 8, 8, 4, 7, 4, 1>()}},    // s3 input conv dgrad (100 -> 50)
    // wide deep space S=(3,4,5), kernels (64, 128, 256): the whole Cin patch in LDS (up to 154 KB: one
    // workgroup of 8 waves per CU for stages 2-3), 2 co tiles x 4 pixel groups per wave
    {8, 8, {tile<5, 5, 1, 32, 8, 4, 8, 4, 1>()}},    // s1 input conv (3 -> 64)
    // s1 nodes / output conv, and their dgrad (64 -> 64): one co tile per wave (-0.7 % per wide step)
    {4, 4, {ct1<3, 3, 8, 32, 4, 4, 8, 4, 0>()}},
    // stage 2 (s2 input conv 64 -> 128; nodes / output conv and their dgrad 128 -> 128): one co tile per wave
    // over all 8 pixel groups (-4.3 % per wide population step, r5/conv_s2n_ct1_ab_r5.txt)
    {8, 8, {ct1<5, 5, 8, 16, 8, 8, 16, 8, 0>()}},
    {8, 8, {ct1<3, 3, 16, 16, 8, 8, 16, 8, 0>()}},
    {4, 4, {tile<5, 5, 16, 16, 4, 4, 8, 4, 1>()}},     // s2 input conv dgrad (128 -> 64)
    {8, 8, {tile<5, 5, 16, 8, 8, 16, 32, 8, 1>()}},    // s3 input conv (128 -> 256)
    {8, 8, {tile<3, 3, 32, 8, 8, 16, 32, 8, 1>()}},    // s3 nodes / output conv, and their dgrad (256 -> 256)
    {4, 4, {tile<5, 5, 32, 8, 4, 8, 16, 4, 1>()}},     // s3 input conv dgrad (256 -> 128)
    // --- bf16 ---
    // Genetic-CNN CIFAR-shaped S=(3,5) space, kernels (20, 50), 5x5 stage convs
    {8, 8, {tile<5, 5, 1, 32, 8, 2, 3, 4, 0>()}},      // s1 input conv (3 -> 20)
    {8, 8, {tile<3, 3, 3, 32, 8, 2, 3, 4, 0>()}},      // s1 nodes / output conv, and their dgrad (20 -> 20)
    {16, 16, {tile<5, 5, 3, 16, 16, 4, 7, 4, 0>()}},   // s2 input conv (20 -> 50)
    {16, 16, {tile<3, 3, 7, 16, 16, 4, 7, 8, 0>()}},   // s2 nodes / output conv, and their dgrad (50 -> 50): 8 waves
    {16, 16, {tile<5, 5, 7, 16, 16, 2, 3, 4, 0>()}},   // s2 input conv dgrad (50 -> 20)
    // deep S=(3,4,5) space, kernels (20, 50, 100): stage 3 at 8x8 (one image per workgroup)
    // (odd tile counts, 104 channels = 7 x 16: one co tile per wave, NT waves)
    {8, 8, {tile<5, 5, 7, 8, 8, 7, 13, 7, 0>()}},      // s3 input conv (50 -> 100)
    {8, 8, {tile<3, 3, 13, 8, 8, 7, 13, 7, 0>()}},     // s3 nodes / output conv, and their dgrad (100 -> 100)
    {8, 8, {tile<5, 5, 13, 8, 8, 4, 7, 4, 0>()}},      // s3 input conv dgrad (100 -> 50)
  };
  return rows;
}

// ---------------------------------------------------------------------------
// selection: arguments -> instantiation and launch geometry (pure; no GPU needed)
// ---------------------------------------------------------------------------
struct ConvChoice {
  const ConvKernel* k;
  dim3 grid;
  unsigned block;
  size_t lds;
};

static bool variant_ok(const ConvArgs* a, const ConvRow& r, const ConvVariant& v) {
  return (!(v.cond & IF_TH) || smallq_th(a, r.hmod, r.thmin) == v.k.TH) && (!(v.cond & IF_PK) || pk_ok(a, v.k.NT)) &&
         (!(v.cond & IF_RE) || g_fast.regepi) && (!(v.cond & IF_S2CT1) || g_fast.s2in_ct1) &&
         (!(v.cond & IF_TWO) || a->twopass);
}

// the search-space rows, then the user-chosen ones: the first row and variant whose condition holds
static bool select_conv(const ConvArgs* a, ConvChoice* c) {
  if (a->mask) return false;                 // staged ReLU mask: generic kernel only
  for (const std::vector<ConvRow>* rows : {&conv_rows(), &conv_rows_ext()})
    for (const ConvRow& r : *rows) {
      const ConvKernel& g = r.v[0].k;
      if (a->KH != g.KH || a->KW != g.KW || a->Cinp != g.NCBI * 8 || a->W != g.W || a->Coutp != g.NCO * 8 ||
          a->prec != g.PREC || a->H % r.hmod != 0)
        continue;
      for (const ConvVariant& v : r.v)
        if (variant_ok(a, r, v)) {
          *c = {&v.k, dim3(a->B * (a->H / v.k.TH), a->ngroups), (unsigned)v.k.NWV * 64,
                (size_t)(a->epi_bf16 != 0 ? v.k.lds_fwd : v.k.lds_bwd)};
          return true;
        }
    }
  return false;
}

// every kernel takes its argument struct by value
static int launch_fast(const void* fn, dim3 grid, unsigned block, size_t lds, const void* args, hipStream_t stream) {
  lds_limit(fn, lds);
  void* kargs[] = {const_cast<void*>(args)};
  (void)hipLaunchKernel(fn, grid, dim3(block), kargs, lds, stream);
  return (int)hipGetLastError();
}

extern "C" int gt_conv_wino(const ConvArgs* a, hipStream_t stream, int probe);

// -100 = no match (the caller then uses the generic kernel)
extern "C" int gt_conv_fast(const ConvArgs* a, hipStream_t stream) {
  if (a->wino) return gt_conv_wino(a, stream, 0);   // Winograd 3x3 layers (cnn_conv_wino.hip)
  if (a->mask) return -100;
  if (a->prec != 0 && a->prec != 1) return -1;
  ConvChoice c;
  if (!select_conv(a, &c)) return -100;
  return launch_fast(c.k->fn, c.grid, c.block, c.lds, a, stream);
}

// tile rows of the kernel gt_conv_fast would launch for these arguments, or 0
static int probe_rows(const ConvArgs* a) {
  if (a->wino) {
    const int rc = gt_conv_wino(a, nullptr, 1);
    return rc >= 1000 ? rc - 1000 : 0;
  }
  ConvChoice c;
  return select_conv(a, &c) ? c.k->TH : 0;
}

// rows of the shape-specialised tile gt_conv_fast would launch for these
// arguments when that kernel can fuse the 2x2 pool (even rows), else 0
extern "C" int gt_conv_fast_probe(const ConvArgs* a) {
  const int th = probe_rows(a);
  return th % 2 == 0 ? th : 0;
}

// 1 when gt_conv_fast would run these (data-gradient) arguments on a
// shape-specialised kernel, which can un-pool its output (fused pool backward)
extern "C" int gt_conv_fast_probe_any(const ConvArgs* a) { return probe_rows(a) > 0 ? 1 : 0; }

// the choice of select_conv as ints (ConvSel of gentun_amd/ops/cnn_kernels.py); returns 1, or 0 for no match
// (Winograd layers included: they run none of these kernels)
struct ConvSel {
  int KH, KW, NCBI, W, TH, NT, NCO, NWV, PREC, PK, RE, CTX, SCH, lds_fwd, lds_bwd;
  int gx, gy, gz, block, lds;
};
extern "C" int gt_conv_fast_select(const ConvArgs* a, ConvSel* s) {
  ConvChoice c;
  if (a->wino || (a->prec != 0 && a->prec != 1) || !select_conv(a, &c)) return 0;
  const ConvKernel& k = *c.k;
  *s = {k.KH, k.KW, k.NCBI, k.W, k.TH, k.NT, k.NCO, k.NWV, k.PREC, k.PK, k.RE, k.CTX, k.SCH, k.lds_fwd, k.lds_bwd,
        (int)c.grid.x, (int)c.grid.y, (int)c.grid.z, (int)c.block, (int)c.lds};
  return 1;
}
extern "C" size_t gt_sizeof_conv_sel() { return sizeof(ConvSel); }

// 1 when gt_conv_fast would run these arguments on a two-pass staging kernel (ConvSel has no room for the
// flag), 0 on another shape-specialised kernel, -1 for no match. The executor probes with twopass = 1.
extern "C" int gt_conv_fast_twopass(const ConvArgs* a) {
  ConvChoice c;
  if (a->wino || (a->prec != 0 && a->prec != 1) || !select_conv(a, &c)) return -1;
  return c.k->TWO;
}

// workgroups of the kernel gt_conv_fast would launch that fit one CU at its registers, LDS and block size
// (hipOccupancyMaxActiveBlocksPerMultiprocessor; needs a GPU), or -1
extern "C" int gt_conv_fast_occupancy(const ConvArgs* a) {
  ConvChoice c;
  int n = 0;
  if (a->wino || (a->prec != 0 && a->prec != 1) || !select_conv(a, &c)) return -1;
  lds_limit(c.k->fn, c.lds);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, c.k->fn, (int)c.block, c.lds) != hipSuccess) return -1;
  return n;
}

__global__ void __launch_bounds__(256) wgrad_reduce_kernel(WgradArgs a) {
  const GroupRec gr = group_rec(a.gtab, blockIdx.y, a.n_in, 0, 0, nullptr);
  const int g = gr.g;
  const long kd = (long)a.KH * a.KW * a.Cinp;
  const long n = (long)a.Coutp * kd;
  const long gs = (long)a.G * n;                   // split stride of part_w
  float* pw = a.part_w + (long)g * n;
  const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 < n) {                                    // n % 4 == 0 (Cinp % 8 == 0)
    // 8 partials in flight per batch (a dependent load-add chain waited for
    // each one: ~20 us per call); summed in split order
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int sp = 0;
    for (; sp + 8 <= a.S; sp += 8) {
      float4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const float4*>(pw + (long)(sp + k) * gs + i4);
#pragma unroll
      for (int k = 0; k < 8; ++k) { acc.x += v[k].x; acc.y += v[k].y; acc.z += v[k].z; acc.w += v[k].w; }
    }
    for (; sp < a.S; ++sp) {
      const float4 v = *reinterpret_cast<const float4*>(pw + (long)sp * gs + i4);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(pw + i4) = acc;
  }
  if (blockIdx.x == 0 && a.part_b) {
    float* pb = a.part_b + (long)g * a.Coutp;
    for (int i = threadIdx.x; i < a.Coutp; i += 256) {
      float acc = 0.f;
      for (int sp = 0; sp < a.S; ++sp) acc += pb[(long)sp * a.G * a.Coutp + i];
      pb[i] = acc;
    }
  }
}

extern "C" int gt_wgrad_reduce(const WgradArgs* a, hipStream_t stream) {
  const long n = (long)a->Coutp * a->KH * a->KW * a->Cinp;
  if (n % 4 || a->S < 2) return -1;
  dim3 grid((unsigned)((n / 4 + 255) / 256), a->ngroups);
  hipLaunchKernelGGL(wgrad_reduce_kernel, grid, dim3(256), 0, stream, *a);
  return (int)hipGetLastError();
}

extern "C" int gt_wgrad_set_nb(int nb) { return swap_switch(g_fast.wgrad_nb, nb); }

// Small launches (few groups x splits: a population job of 1-5 groups, the
// reference's sequential folds or a rank's share on 8 GPUs): the k-column
// tiles are sliced over NZ workgroups that stage the same bands, so the
// grid fills more CUs and each workgroup's serial band loop carries 1/NZ of
// the MFMAs. Every weight's sum runs in the same band / k-step order in any
// slice: results are bit-identical for any NZ (tests/test_hip_kernels.py).
// gt_wgrad_set_nz (tests): 0 auto (default), 1 / 2 / 4 / 8 forced (8: 4-wave workgroups).
extern "C" int gt_wgrad_set_nz(int nz) { return swap_switch(g_fast.wgrad_nz, nz); }

static int wgrad_nz(const WgradArgs* a) {
  const int force = g_fast.wgrad_nz;
  if (force == 1 || force == 2 || force == 4 || force == 8) return force;
  // (an 8-slice variant below ~32 blocks measured neutral at 2 groups: profiles/wgrad_nz8_ab_r4.txt)
  const int blocks = a->S * a->ngroups;
  return blocks < 64 ? 4 : blocks < 160 ? 2 : 1;
}

// packed last co tile of the fp32 wgrad
static bool wgrad_pk_ok(const WgradArgs* a, int mt) {
  const int last = a->cout_real - 16 * (mt - 1);
  return a->cout_real > 0 && last >= 1 && last <= 4;
}

// wgrad shape table: <KH, KW, NCBI, NCBO, W, R, NW, NB> (wgrad_f32z: NZ last). The host sizes the split in
// whole bands of R rows (gt_wgrad_fast_band)
static const std::vector<WgradRow>& wgrad_rows() {
  static const std::vector<WgradRow> rows = {
    wgrad_f32<5, 5, 1, 3, 32, 8, 4, 1>(),      // s1 input conv (3 -> 20)
    wgrad_f32<3, 3, 3, 3, 32, 4, 4, 1>(),      // s1 nodes / output conv (20 -> 20)
    // s2: ONE band buffer (57 KB of LDS instead of 115): in the population step the wgrads run beside the
    // data-gradient convs, and a single-buffered wgrad workgroup leaves room on its CU for a conv
    // workgroup (60 KB) -- 1.1-1.6 % per step from 25 groups up although the wgrad alone is slower
    // (profiles/wgrad_nb_ab_r4.txt)
    wgrad_f32<5, 5, 3, 7, 16, 4, 8, 1>(),      // s2 input conv (20 -> 50)
    wgrad_f32<3, 3, 7, 7, 16, 4, 8, 1>(),      // s2 nodes / output conv (50 -> 50)
    wgrad_f32z<5, 5, 7, 13, 8, 4, 8, 4>(),     // deep s3 input conv (50 -> 100)
    wgrad_f32z<3, 3, 13, 13, 8, 4, 8, 4>(),    // deep s3 nodes / output conv (100 -> 100)
    // wide deep space (64, 128, 256): column slices so each workgroup's dW slice fits its registers
    wgrad_f32<5, 5, 1, 8, 32, 4, 4, 1>(),      // s1 input conv (3 -> 64)
    wgrad_f32<3, 3, 8, 8, 32, 2, 8, 1>(),      // s1 nodes / output conv (64 -> 64)
    wgrad_f32z<5, 5, 8, 16, 16, 2, 8, 7>(),    // s2 input conv (64 -> 128)
    wgrad_f32z<3, 3, 16, 16, 16, 2, 8, 4>(),   // s2 nodes / output conv (128 -> 128)
    wgrad_f32z<5, 5, 16, 32, 8, 4, 8, 13>(),   // s3 input conv (128 -> 256)
    wgrad_f32z<3, 3, 32, 32, 8, 4, 8, 10>(),   // s3 nodes / output conv (256 -> 256)
    wgrad_bf16<5, 5, 1, 3, 32, 8, 4, 1>(),     // s1 input conv (3 -> 20)
    wgrad_bf16<3, 3, 3, 3, 32, 8, 4, 1>(),     // s1 nodes / output conv (20 -> 20)
    wgrad_bf16<5, 5, 3, 7, 16, 16, 8, 2>(),    // s2 input conv (20 -> 50)
    wgrad_bf16<3, 3, 7, 7, 16, 16, 8, 2>(),    // s2 nodes / output conv (50 -> 50)
  };
  return rows;
}

// the row of a layer geometry (the search-space rows, then the user-chosen ones), or null
static const WgradRow* wgrad_row(int KH, int KW, int Cinp, int Coutp, int H, int W, int prec) {
  for (const std::vector<WgradRow>* rows : {&wgrad_rows(), &wgrad_rows_ext()})
    for (const WgradRow& r : *rows)
      if (KH == r.KH && KW == r.KW && Cinp == r.NCBI * 8 && Coutp == r.NCBO * 8 && W == r.W && prec == r.PREC &&
          H % r.R == 0)
        return &r;
  return nullptr;
}

struct WgradChoice {
  const WgradKernel* k;
  dim3 grid;
  unsigned block;
};

static bool select_wgrad(const WgradArgs* a, WgradChoice* c) {
  const WgradRow* r = wgrad_row(a->KH, a->KW, a->Cinp, a->Coutp, a->H, a->W, a->prec);
  if (!r || a->pps % (r->R * r->W) != 0) return false;
  const int nz = r->NZ ? r->NZ : wgrad_nz(a);
  const int pk = r->PREC == 1 && wgrad_pk_ok(a, (r->NCBO * 8 + 15) / 16) ? 1 : 0;
  int nw = r->NW, nb = 1;
  // automatic slices: 2 keep the shape's band buffers (2 for a 16-wide stage: its 2 x S x G workgroups fit one
  // per CU), 8 (tiny launches, < 32 split x group blocks) run 4-wave workgroups; fixed slices: one band buffer
  if (r->NZ == 0 && nz == 2) nb = r->NB;
  else if (r->NZ == 0 && nz == 8) nw = 4;
  else if (nz == 1) nb = (g_fast.wgrad_nb ? g_fast.wgrad_nb : r->NB) == 1 ? 1 : 2;
  for (const WgradKernel& k : r->k)
    if (k.NW == nw && k.NB == nb && k.PK == pk && k.NZ == nz) {
      *c = {&k, dim3(a->S, a->ngroups, nz), (unsigned)nw * 64};
      return true;
    }
  return false;
}

// pixels per band of the specialised wgrad for this geometry (the host sizes the split in whole bands), or 0
extern "C" int gt_wgrad_fast_band(int KH, int KW, int Cinp, int Coutp, int H, int W, int prec) {
  const WgradRow* r = wgrad_row(KH, KW, Cinp, Coutp, H, W, prec);
  return r ? r->R * r->W : 0;
}

// Preferred splits per group (measured, profiles/wgrad_splits.txt): many small
// workgroups for the 32-wide stage (single LDS buffer, 4+ per CU), few large
// ones for the 16-wide stage (double-buffered: 128 KB of LDS, one workgroup per
// CU). 3 splits x 80 groups of a 16-candidate population = 240 workgroups, one
// round on 256 CUs; 4 splits left a 64-workgroup second round (population step
// 2-3 % slower, same-box sweep).
// fp32 (prec 1): the band work is ~6x the bf16 one, and a bench round
// trains only ~10 groups per launch: 8 / 32 splits keep >= 80 / 320
// workgroups busy at 10 groups (3 splits left 30 workgroups on 256 CUs:
// 199 us per call, 34 % of a 10-group step) for 2.7x the partial-sum bytes.
extern "C" int gt_wgrad_fast_splits(int KH, int KW, int Cinp, int Coutp, int H, int W, int prec) {
  (void)KH; (void)KW; (void)Cinp; (void)Coutp; (void)H;
  if (prec == 1) {
    // 8-wide (deep stage 3): 4 splits x 4 column slices per group
    // (12 or 16 splits for the 16-wide stage: 0.4-1.8 % slower steps at 25 and 80 groups,
    // profiles/r5/wgrad_splits_ab_r5.txt)
    return W >= 32 ? 32 : W <= 8 ? 4 : 8;
  }
  return W >= 32 ? 16 : 3;
}

extern "C" int gt_wgrad_fast(const WgradArgs* a, hipStream_t stream) {
  if (a->prec != 0 && a->prec != 1) return -1;
  WgradChoice c;
  if (!select_wgrad(a, &c)) return -100;
  return launch_fast(c.k->fn, c.grid, c.block, 0, a, stream);
}

// the choice of select_wgrad as ints (WgradSel of gentun_amd/ops/cnn_kernels.py); returns 1, or 0 for no match
struct WgradSel {
  int KH, KW, NCBI, NCBO, W, R, NW, NB, PK, NZ, PREC;
  int gx, gy, gz, block, lds;
};
extern "C" int gt_wgrad_fast_select(const WgradArgs* a, WgradSel* s) {
  WgradChoice c;
  if (!select_wgrad(a, &c)) return 0;
  const WgradKernel& k = *c.k;
  *s = {k.KH, k.KW, k.NCBI, k.NCBO, k.W, k.R, k.NW, k.NB, k.PK, k.NZ, k.PREC,
        (int)c.grid.x, (int)c.grid.y, (int)c.grid.z, (int)c.block, 0};
  return 1;
}
extern "C" size_t gt_sizeof_wgrad_sel() { return sizeof(WgradSel); }

// ===========================================================================
// Fragment-major weight planes of the shape-specialised convs (ConvArgs::wfrag)
// ===========================================================================
// Entry e of a conv's reduction list -> its row-major chunk (kk * NCBI + cb), as the kernels order it
// (part-major for the stage-2 3x3 fp32 shape, S2Parts; kk-major otherwise); -1 past the list.
extern "C" int gt_conv_frag_order(int KH, int KW, int NCBI, int W, int prec, int* out, int n) {
  const int NCH = KH * KW * NCBI;
  const bool parts = prec == 1 && NCBI == 7 && W == 16 && KH == 3 && KW == 3;
  for (int e = 0; e < n; ++e) {
    int kk, cb;
    if (e >= NCH) { out[e] = -1; continue; }
    if (parts) {
      const int E0 = KH * KW * 4;
      if (e < E0) { kk = e >> 2; cb = e & 3; }
      else { const int e1 = e - E0; kk = e1 / 3; cb = 4 + e1 - kk * 3; }
    } else {
      kk = e / NCBI; cb = e - kk * NCBI;
    }
    out[e] = kk * NCBI + cb;
  }
  return (NCH + 3) / 4;
}

struct FragSeg {
  const float* w;        // fp32 master [Q][Cop][KH][KW][Cip] of the layer
  uint16_t* dst;         // [npl][Q][NT][NKS][64][8] bf16 planes
  const int* order;      // [NKS * 4]: row-major chunk of each entry in the conv's view, -1 = zero
  long ps;               // plane stride (elements)
  int Q, Cop, Cip, KH, KW;
  int NT, NKS, NCBIc;    // the conv's co tiles, k-steps, input chunks (layer Cip / 8, or Cop / 8 for dgrad)
  int dgrad;             // 1: the flipped / transposed kernel of the data gradient
  int npl;               // 3 (fp32: exact split) or 1 (bf16)
};

struct FragArgs {
  const FragSeg* segs;
  const int2* blocks;    // per block: (segment, first lane-item of Q x NT x NKS x 64)
};

__global__ void __launch_bounds__(256) conv_wfrag_kernel(FragArgs a) {
  const int2 blk = a.blocks[blockIdx.x];
  const FragSeg s = a.segs[blk.x];
  const long item = (long)blk.y + threadIdx.x;
  if (item >= (long)s.Q * s.NT * s.NKS * 64) return;
  const int lane = (int)(item & 63);
  long r = item >> 6;
  const int ks = (int)(r % s.NKS); r /= s.NKS;
  const int t = (int)(r % s.NT);
  const int q = (int)(r / s.NT);
  const int row = t * 16 + (lane & 15), e = ks * 4 + (lane >> 4);
  const int nat = s.order[e];
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  if (nat >= 0) {
    const int kk = nat / s.NCBIc, cb = nat - kk * s.NCBIc;
    const int kh = kk / s.KW, kw = kk - kh * s.KW;
    if (!s.dgrad && row < s.Cop) {
      const float* src = s.w + ((((long)q * s.Cop + row) * s.KH + kh) * s.KW + kw) * s.Cip + cb * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[j];
    } else if (s.dgrad && row < s.Cip) {
      // the data gradient's row = layer input channel, its chunk cb = layer output channels cb*8.., flipped taps
      const int khl = s.KH - 1 - kh, kwl = s.KW - 1 - kw;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = s.w[((((long)q * s.Cop + cb * 8 + j) * s.KH + khl) * s.KW + kwl) * s.Cip + row];
    }
  }
  uint16_t* d = s.dst + item * 8;
  if (s.npl == 1) {
    *reinterpret_cast<uint4*>(d) = pack8(v);
    return;
  }
  uint4 p0, p1, p2;
  split8(v, p0, p1, p2);
  *reinterpret_cast<uint4*>(d) = p0;
  *reinterpret_cast<uint4*>(d + s.ps) = p1;
  *reinterpret_cast<uint4*>(d + 2 * s.ps) = p2;
}

extern "C" int gt_conv_wfrag(const void* av, int nblocks, hipStream_t stream) {
  if (nblocks < 1) return 0;
  hipLaunchKernelGGL(conv_wfrag_kernel, dim3(nblocks), dim3(256), 0, stream, *static_cast<const FragArgs*>(av));
  return (int)hipGetLastError();
}

extern "C" size_t gt_sizeof_frag_seg() { return sizeof(FragSeg); }
