// Shape-specialised conv / weight-gradient rows for user-chosen architectures (the reference lets the
// user pick kernels_per_layer and kernel_sizes, gentun/individuals.py:221-223): 32 / 64-channel stages
// (kernels (32, 64) -- padding them up to the wide (64, 128) shapes cost 4x the multiply-adds and ran slower
// than the generic kernels, profiles/r6/generality_r6.txt) and 3x3 stage-input convs, each tiled like its
// (20, 50) / 5x5 counterpart. Its own translation unit (compiled in parallel with cnn_conv_fast.hip), which
// only holds table rows: selection, launch and the switches are cnn_conv_fast.hip's (row types: conv_fast_host.h).
#include "conv_fast_host.h"

const std::vector<ConvRow>& conv_rows_ext() {
  static const std::vector<ConvRow> rows = {
    // 32 / 64-channel stages, tiled like the (20, 50) shapes
    {8, 4, {tile<5, 5, 1, 32, 4, 2, 4, 2, 1>(IF_TH), tile<5, 5, 1, 32, 8, 2, 4, 4, 1>()}},   // s1 input conv (3 -> 32)
    {8, 4, {tile<3, 3, 1, 32, 4, 2, 4, 2, 1>(IF_TH), tile<3, 3, 1, 32, 8, 2, 4, 4, 1>()}},   // s1 input conv 3x3 (3 -> 32)
    // s1 nodes / output conv and their dgrad (32 -> 32)
    {8, 4, {tile<3, 3, 4, 32, 4, 2, 4, 2, 1>(IF_TH), tile<3, 3, 4, 32, 8, 2, 4, 4, 1>()}},
    // s2 input conv (32 -> 64)
    {8, 2, {tile<5, 5, 4, 16, 4, 4, 8, 4, 1>(IF_TH), ct1<5, 5, 4, 16, 2, 4, 8, 4>(IF_TH), ct1<5, 5, 4, 16, 8, 4, 8, 4, 0>()}},
    // s2 input conv 3x3 (32 -> 64)
    {8, 2, {tile<3, 3, 4, 16, 4, 4, 8, 4, 1>(IF_TH), ct1<3, 3, 4, 16, 2, 4, 8, 4>(IF_TH), ct1<3, 3, 4, 16, 8, 4, 8, 4, 0>()}},
    // s2 nodes / output conv and their dgrad (64 -> 64)
    {8, 2, {tile<3, 3, 8, 16, 4, 4, 8, 4, 1>(IF_TH), ct1<3, 3, 8, 16, 2, 4, 8, 4>(IF_TH), ct1<3, 3, 8, 16, 8, 4, 8, 4, 0>()}},
    {8, 4, {ct1<5, 5, 8, 16, 4, 2, 4, 4>(IF_TH), ct1<5, 5, 8, 16, 8, 2, 4, 4>()}},   // s2 input conv dgrad (64 -> 32)
    {8, 4, {ct1<3, 3, 8, 16, 4, 2, 4, 4>(IF_TH), ct1<3, 3, 8, 16, 8, 2, 4, 4>()}},   // s2 input conv 3x3 dgrad (64 -> 32)
    // 3x3 stage-input kernels (kernel_sizes ((3, 3), ...): a user choice, gentun/individuals.py:223), tiled
    // like their 5x5 counterparts; the 3x3 node shapes are the same kernels already
    {8, 4, {tile<3, 3, 1, 32, 4, 2, 3, 2, 1, 1>(IF_TH | IF_PK), tile<3, 3, 1, 32, 4, 2, 3, 2, 1>(IF_TH),
            tile<3, 3, 1, 32, 8, 2, 3, 4, 1, 1>(IF_PK), tile<3, 3, 1, 32, 8, 2, 3, 4, 1>()}},   // s1 input conv 3x3 (3 -> 20)
    // s2 input conv 3x3 (20 -> 50)
    {8, 2, {tile<3, 3, 3, 16, 4, 4, 7, 4, 1>(IF_TH), ct1<3, 3, 3, 16, 2, 4, 7, 4>(IF_TH), ct1<3, 3, 3, 16, 8, 4, 7, 4, 0>()}},
    {8, 4, {ct1<3, 3, 7, 16, 4, 2, 3, 4>(IF_TH), ct1<3, 3, 7, 16, 8, 2, 3, 4>()}},   // s2 input conv 3x3 dgrad (50 -> 20)
    {8, 8, {tile<3, 3, 7, 8, 8, 7, 13, 7, 1>()}},      // deep s3 input conv 3x3 (50 -> 100)
    {8, 8, {tile<3, 3, 13, 8, 8, 4, 7, 4, 1>()}},      // deep s3 input conv 3x3 dgrad (100 -> 50)
    {8, 8, {tile<3, 3, 1, 32, 8, 4, 8, 4, 1>()}},      // wide s1 input conv 3x3 (3 -> 64)
    {8, 8, {ct1<3, 3, 8, 16, 8, 8, 16, 8, 0>()}},      // wide s2 input conv 3x3 (64 -> 128)
    {4, 4, {tile<3, 3, 16, 16, 4, 4, 8, 4, 1>()}},     // wide s2 input conv 3x3 dgrad (128 -> 64)
    {8, 8, {tile<3, 3, 16, 8, 8, 16, 32, 8, 1>()}},    // wide s3 input conv 3x3 (128 -> 256)
    {4, 4, {tile<3, 3, 32, 8, 4, 8, 16, 4, 1>()}},     // wide s3 input conv 3x3 dgrad (256 -> 128)
  };
  return rows;
}

const std::vector<WgradRow>& wgrad_rows_ext() {
  static const std::vector<WgradRow> rows = {
    // 32 / 64-channel stages
    wgrad_f32<5, 5, 1, 4, 32, 8, 4, 1>(),      // s1 input conv (3 -> 32)
    wgrad_f32<3, 3, 1, 4, 32, 8, 4, 1>(),      // s1 input conv 3x3 (3 -> 32)
    wgrad_f32<3, 3, 4, 4, 32, 4, 4, 1>(),      // s1 nodes / output conv (32 -> 32)
    wgrad_f32z<5, 5, 4, 8, 16, 4, 8, 2>(),     // s2 input conv (32 -> 64)
    wgrad_f32<3, 3, 4, 8, 16, 4, 8, 1>(),      // s2 input conv 3x3 (32 -> 64)
    wgrad_f32<3, 3, 8, 8, 16, 4, 8, 1>(),      // s2 nodes / output conv (64 -> 64)
    // 3x3 stage-input kernels (bands as their 5x5 counterparts)
    wgrad_f32<3, 3, 1, 3, 32, 8, 4, 1>(),      // s1 input conv 3x3 (3 -> 20)
    wgrad_f32<3, 3, 3, 7, 16, 4, 8, 1>(),      // s2 input conv 3x3 (20 -> 50)
    wgrad_f32z<3, 3, 7, 13, 8, 4, 8, 4>(),     // deep s3 input conv 3x3 (50 -> 100)
    wgrad_f32<3, 3, 1, 8, 32, 4, 4, 1>(),      // wide s1 input conv 3x3 (3 -> 64)
    wgrad_f32z<3, 3, 8, 16, 16, 2, 8, 4>(),    // wide s2 input conv 3x3 (64 -> 128)
    wgrad_f32z<3, 3, 16, 32, 8, 4, 8, 5>(),    // wide s3 input conv 3x3 (128 -> 256)
  };
  return rows;
}
