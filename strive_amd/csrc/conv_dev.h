// Device blocks of the "fp16 x 3" convolutions (conv2 .. conv4): the tile geometry (BfCfg) and the arithmetic that
// conv_bf6_kernel, conv_ws_kernel and conv_wsx_kernel (map_cnn.hip) are all written on.  The three kernel forms stage, multiply
// and reduce through these functions and through nothing else, so "same products in the same order" -- bit-identical outputs and
// GroupNorm moments whatever form runs a layer -- is a property of the code, not of copies kept in step.
// conv_bf6s_kernel and map_cnn_tail.h (small images, linearised pixels) share the fp16 split and the moments arithmetic only.
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

#define GN_EPS 1e-5

struct GNStats { double sum, sq; };

// =============================================================================================
// GroupNorm(1 group) of the producing layer, applied while the consumer stages its input
// =============================================================================================
__device__ __forceinline__ void gn_mean_rstd(double s, double q, double count, float& mean, float& rstd) {
    const double m = s / count;
    double var = q / count - m * m;
    var = var < 0.0 ? 0.0 : var;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + GN_EPS));
}

// Per-sample GroupNorm(1) moments from the producing layer's per-tile partial sums, added in tile order
// (no atomics anywhere: the CNN is bitwise reproducible run to run, which matters because the rollout
// re-samples the raster at poses that depend on these features).
__device__ __forceinline__ void gn_moments(const GNStats* __restrict__ st, int n, int nparts, double count, float& mean,
                                           float& rstd) {
    double s = 0.0, q = 0.0;
    for (int i = 0; i < nparts; ++i) {
        s += st[(size_t)n * nparts + i].sum;
        q += st[(size_t)n * nparts + i].sq;
    }
    gn_mean_rstd(s, q, count, mean, rstd);
}

// The same moments by one wave: the partial sums one per lane, reduced in a fixed (butterfly) order; every lane gets them
template <class Cfg>
__device__ __forceinline__ void gn_moments_wave(const GNStats* __restrict__ st_in, int n, int lane, float& mean, float& rstd) {
    double ps = 0.0, pq = 0.0;
    for (int i = lane; i < Cfg::NPART_IN; i += 64) {
        ps += st_in[(size_t)n * Cfg::NPART_IN + i].sum;
        pq += st_in[(size_t)n * Cfg::NPART_IN + i].sq;
    }
    ps = wave_sum_d(ps);
    pq = wave_sum_d(pq);
    gn_mean_rstd(ps, pq, (double)Cfg::CIN * Cfg::IH * Cfg::IH, mean, rstd);
}

// scale, shift of one channel -> dst[0], dst[1].  xscale = 2^k folded into the affine map:
// relu(2^k (a x + b)) = 2^k relu(a x + b), exact
__device__ __forceinline__ void gn_affine(float mean, float rstd, float g, float b, float xscale, float* dst) {
    const float sc = rstd * g;
    dst[0] = sc * xscale;
    dst[1] = (b - mean * sc) * xscale;
}

// one wave: scale / shift of every input channel of sample n -> s_gn[CIN][2]
template <class Cfg>
__device__ __forceinline__ void gn_scale_shift(const GNStats* __restrict__ st_in, int n, const float* __restrict__ gn_g,
                                               const float* __restrict__ gn_b, float xscale, int lane, float* s_gn) {
    float mean, rstd;
    gn_moments_wave<Cfg>(st_in, n, lane, mean, rstd);
    if (lane < Cfg::CIN) gn_affine(mean, rstd, gn_g[lane], gn_b[lane], xscale, s_gn + 2 * lane);
}

// =============================================================================================
// Tile geometry of layers 2-4 (the scheme, the LDS layout and the k order are described at conv_bf6_kernel in map_cnn.hip)
// =============================================================================================
template <int CIN_, int COUT_, int KS_, int IH_, int OH_, int NPART_IN_, bool OUT_OCT_, int PT_ = 2, int WGS_PER_CU_ = 2,
          bool ROWS2_ = false, int CBW_ = 1>
struct BfCfg {
    static constexpr int CIN = CIN_, COUT = COUT_, KS = KS_, IH = IH_, OH = OH_, NPART_IN = NPART_IN_;
    static constexpr bool OUT_OCT = OUT_OCT_;
    static constexpr int PT = PT_;                                  // pixel tiles of 32 per wave
    static constexpr bool ROWS2 = ROWS2_;                           // pixel tile = 2 rows x 16 columns (small images) instead of 1 x 32
    static constexpr int TILE_ROWS = ROWS2 ? 2 : 1;
    static constexpr int WGS_PER_CU = WGS_PER_CU_;                  // residency target (LDS and register budget)
    static constexpr int NT = 256, NW = 4, TH = NW * PT * TILE_ROWS, TW = ROWS2 ? 16 : 32;
    // a workgroup computes CBW blocks of 32 output channels from ONE staging of the input tile (the matrix steps of a pass
    // run once per block): the input is fetched, normalised and split COUT / (32 CBW) times instead of COUT / 32 times
    static constexpr int CBW = CBW_, COUT_WG = 32 * CBW, CSPLIT = COUT / COUT_WG;
    static constexpr int PASS_CH = 8, NPASS = CIN / PASS_CH;
    static constexpr int ITH = 2 * TH + KS - 2, ITW = 2 * TW + KS - 2, HW = (ITW + 1) / 2;
    static constexpr int HALF_B = HW * 16, ROW_B = 2 * HALF_B, PIECE_B = ITH * ROW_B;
    static constexpr int NPIECE = 2;                                          // fp16 pieces per value
    static constexpr int IN_B = (NPIECE * PIECE_B + 255) / 256 * 256;         // weight fragments start 256-byte aligned
    static constexpr int NKS = (KS * KS + 1) / 2;                            // MFMA steps per pass (two taps each)
    static constexpr int WSTEP_B = CBW * 2 * 64 * 16;                        // one matrix step: [block][piece][lane][16 B]
    static constexpr int TILES_X = (OH + TW - 1) / TW, TILES_Y = (OH + TH - 1) / TH;
    static constexpr int NPART_OUT = TILES_X * TILES_Y * CSPLIT;
    static constexpr int UNITS = ITH * ITW, UITERS = (UNITS + NT - 1) / NT;
    static constexpr size_t LDS_BYTES = (size_t)IN_B + 3 * WSTEP_B + (size_t)CIN * 8 + NW * 16 + 16 + COUT_WG * 4;
    static constexpr size_t WFRAG_BYTES = (size_t)NPASS * NKS * (COUT / 32) * 2048;
    // (parameter kept in BfsCfg's position: conv6, a BfsCfg, is the one layer that writes NCHW)
    static_assert(OUT_OCT, "conv2 .. conv4 write octet-planar activations: conv_tile_epilogue has no other store");
    static_assert(CIN % PASS_CH == 0 && COUT % COUT_WG == 0 && CIN <= NT, "channel tiling");
    static_assert(LDS_BYTES * WGS_PER_CU <= 160 * 1024, "LDS budget of the residency target");
    static_assert((KS == 5 && NKS == 13) || (KS == 3 && NKS == 5), "tap orders exist for 5x5 and 3x3 windows");
    static_assert(WSTEP_B == 16 * 128 * CBW && WSTEP_B / 16 <= NT, "weight step = one 16-byte piece for each of the first 128 CBW threads");
    // weight steps of a pass requested before its staging; the rest is requested at matrix step W_LATE_AT, when the registers
    // of the first steps have been handed to LDS.  Three workgroups per CU leave 168 registers per lane: with all 13 steps
    // parked (52 registers) conv2 spilled 11 of them to scratch -- 92 MB written and 92 MB read back per 512-agent launch
    // (rocprofv3 WRITE_SIZE / FETCH_SIZE), a sixth of the kernel's HBM traffic.
    static constexpr int W_UPFRONT = (WGS_PER_CU >= 3 && NKS > 8) ? 7 : NKS, W_LATE_AT = 2;
};

// v = p0 + p1 up to 2^-24 |v| (p0 = fp16(v) rounded to nearest, p1 = fp16(v - p0)); v is pre-scaled into fp16's range.
// Two values per conversion (v_cvt_pk_f16_f32 on gfx950, round to nearest even like the scalar form: same bits, 6 instead of 8
// instructions per pair); the subtraction stays scalar (no packed fp32 arithmetic: DESIGN.md 8.1).
typedef float split_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 split_f16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_f16x2(const float v[8], uint4& p0, uint4& p1) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const split_f32x2 v2 = {v[2 * i], v[2 * i + 1]};
        const split_f16x2v a = __builtin_convertvector(v2, split_f16x2v);
        const float r0 = v[2 * i] - (float)a[0];            // exact
        const float r1 = v[2 * i + 1] - (float)a[1];
        const split_f32x2 r2 = {r0, r1};
        const split_f16x2v c = __builtin_convertvector(r2, split_f16x2v);
        __builtin_memcpy(&h[i], &a, 4);
        __builtin_memcpy(&l[i], &c, 4);
    }
    p0 = make_uint4(h[0], h[1], h[2], h[3]);
    p1 = make_uint4(l[0], l[1], l[2], l[3]);
}

// One staged pixel: the 8 channels of a pass at (row r, column col) of the input tile `buf`.  a, b = the raw fp32 octet,
// g0 .. g3 = (scale, shift) of the 8 channels: GroupNorm + ReLU (pre-scaled), two-piece fp16 split, one 16-byte LDS write per piece.
template <class Cfg>
__device__ __forceinline__ void stage_octet(unsigned char* buf, int r, int col, bool in_image, const float4& a, const float4& b,
                                            const float4& g0, const float4& g1, const float4& g2, const float4& g3) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;             // exact zero outside the image
    if (in_image) {
        v[0] = fmaxf(fmaf(a.x, g0.x, g0.y), 0.f);
        v[1] = fmaxf(fmaf(a.y, g0.z, g0.w), 0.f);
        v[2] = fmaxf(fmaf(a.z, g1.x, g1.y), 0.f);
        v[3] = fmaxf(fmaf(a.w, g1.z, g1.w), 0.f);
        v[4] = fmaxf(fmaf(b.x, g2.x, g2.y), 0.f);
        v[5] = fmaxf(fmaf(b.y, g2.z, g2.w), 0.f);
        v[6] = fmaxf(fmaf(b.z, g3.x, g3.y), 0.f);
        v[7] = fmaxf(fmaf(b.w, g3.z, g3.w), 0.f);
    }
    uint4 p0, p1;
    split_f16x2(v, p0, p1);
    unsigned char* dst = buf + r * Cfg::ROW_B + (col & 1) * Cfg::HALF_B + (col >> 1) * 16;
    *reinterpret_cast<uint4*>(dst) = p0;
    *reinterpret_cast<uint4*>(dst + Cfg::PIECE_B) = p1;
}

// Byte offset, from a lane's window origin, of the tap that lane half h multiplies in matrix step t.
//   5x5: steps 0-9: row ky = t / 2, columns kx = (t & 1) + 2h (same row, same parity: the two 512-byte windows overlap);
//        steps 10-11: column 4 of rows 2 (t - 10) + h;  step 12: tap (4, 4) and one zero-weight slot (row 5 does not exist).
//   3x3: steps 0-2 = row t, columns 0 and 2; step 3 = column 1 of rows 0, 1; step 4 = (2, 1) + zero-weight slot.
template <class Cfg>
__device__ __forceinline__ int conv_tap_offset(int t, int h) {
    int ky, kx;
    if (Cfg::KS == 5) {
        if (t < 10) { ky = t >> 1; kx = (t & 1) + 2 * h; }
        else { ky = 2 * (t - 10) + h; kx = 4; ky = ky > 4 ? 4 : ky; }
    } else {
        if (t < 3) { ky = t; kx = 2 * h; }
        else if (t == 3) { ky = h; kx = 1; }
        else { ky = 2; kx = 1; }
    }
    return ky * Cfg::ROW_B + (kx & 1) * Cfg::HALF_B + (kx >> 1) * 16;
}

// The A (weights: CBW blocks x 2 pieces) and B (input: PT pixel tiles x 2 pieces) fragments of one matrix step.
//   wb: this lane's 16 bytes of the step's first weight fragment ([block][piece][lane][16 B])
//   in: this lane's window origin in piece 0 of the wave's first pixel tile; tile i is 2 TILE_ROWS i input rows further
// (CBW, PT: Cfg's, or conv_ws_kernel's 1 x 1 -- eight consumer waves of one pixel tile each on conv2's geometry)
template <class Cfg, int CBW = Cfg::CBW, int PT = Cfg::PT>
struct ConvFrags {
    f16x8 a[CBW][2], b[PT][2];
    __device__ __forceinline__ void load(const unsigned char* wb, const unsigned char* in, int t, int h) {
        const int off = conv_tap_offset<Cfg>(t, h);
#pragma unroll
        for (int c = 0; c < CBW; ++c)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) a[c][pl] = *reinterpret_cast<const f16x8*>(wb + (c * 2 + pl) * 1024);
#pragma unroll
        for (int i = 0; i < PT; ++i)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
                b[i][pl] = *reinterpret_cast<const f16x8*>(in + pl * Cfg::PIECE_B + 2 * Cfg::TILE_ROWS * i * Cfg::ROW_B + off);
    }
};

// One step of the software pipeline over the matrix steps: while the matrix cores work on step t (fragments `cur`), the
// fragments of step t + 1 are read from LDS into the other register set (`nxt`, from wb_next / in; has_next = false: last step of
// the run).  Three products per (channel block, pixel tile) (w1 x0, w0 x1, w0 x0: the small ones first; w1 x1 is below 2^-24 of
// the leading product); the accumulation chains alternate so that an MFMA never waits for the one issued just before it.
template <class Cfg, int CBW, int PT>
__device__ __forceinline__ void conv_matrix_step(f32x16 (&acc)[CBW][PT], const ConvFrags<Cfg, CBW, PT>& cur, ConvFrags<Cfg, CBW, PT>& nxt,
                                                 bool has_next, const unsigned char* wb_next, const unsigned char* in, int t_next, int h) {
    if (has_next) nxt.load(wb_next, in, t_next, h);
    constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};
#pragma unroll
    for (int term = 0; term < 3; ++term)
#pragma unroll
        for (int c = 0; c < CBW; ++c)
#pragma unroll
            for (int i = 0; i < PT; ++i)
                acc[c][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.a[c][TA[term]], cur.b[i][TB[term]], acc[c][i], 0, 0, 0);
    // issue order pinned: one LDS fragment read of step t+1 behind each MFMA of step t.  Issuing the reads up front stalls the wave
    // on the LDS queue before the matrix pipe gets any work; left to itself (round 6, conv_ws_kernel) the scheduler -- which does
    // not know that the dynamic LDS allocation admits one workgroup per CU, and so minimises registers -- re-reads each weight
    // fragment into ONE register set just before its use: ds_read, s_waitcnt lgkmcnt(0), two matrix instructions, ds_read ... -- an
    // exposed LDS round trip per pair of matrix instructions.  (CBW = PT = 1: MFMA, read, MFMA, read, MFMA, read, read.)
    if (has_next) {
        constexpr int NRD = 2 * CBW + 2 * PT, NMF = 3 * PT * CBW;
#pragma unroll
        for (int q = 0; q < (NRD < NMF ? NRD : NMF); ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // 1 MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // 1 DS read
        }
        if (NMF > NRD) __builtin_amdgcn_sched_group_barrier(0x008, NMF - NRD, 0);
        if (NRD > NMF) __builtin_amdgcn_sched_group_barrier(0x100, NRD - NMF, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int CBW, int PT>
__device__ __forceinline__ void conv_zero_acc(f32x16 (&acc)[CBW][PT]) {
#pragma unroll
    for (int c = 0; c < CBW; ++c)
#pragma unroll
        for (int i = 0; i < PT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][i][r] = 0.f;
}

// Epilogue of a wave's CBW x PT accumulator tiles: D column = lane & 31 = pixel, row = (r & 3) + 8 (r >> 2) + 4 h = channel within
// the block.  out_blk = the first octet plane ([c/8][y][x][c%8]) of the workgroup's channel blocks in this sample, s_bias their
// bias, oy_w = output row of the wave's first pixel tile; (prow, pcol) = this lane's pixel inside a tile.
// The bias comes from LDS, all values of a tile up front (round 6): a global load in the epilogue is waited for with vmcnt(0) (the
// wait-count pass merges the divergent store blocks conservatively), and on gfx9 stores count in vmcnt too: every bias load
// waited for the stores issued before it -- 16 serial store round trips per wave in conv3's epilogue.  Store addresses are a
// uniform 64-bit base + a 32-bit lane offset.
// GroupNorm moments: the 16 outputs of one accumulator tile (one pixel x 16 channels) are summed in fp32, everything above that
// in float64 (added to dsum / dsq).  The fp32 unit is the same set of values in the same order for every tiling of the layer
// (CBW, PT are per-form parameters: DESIGN.md 4.10), so the forms differ only in the grouping of float64 additions: 1e-16, i.e.
// the same fp32 mean and rstd -- a scene decoded alone and inside a large batch gets the same map features.
template <class Cfg, int CBW, int PT>
__device__ __forceinline__ void conv_tile_epilogue(const f32x16 (&acc)[CBW][PT], const float* s_bias, float unscale,
                                                   float* out_blk, int oy_w, int ox0, int prow, int pcol, int h, bool store,
                                                   double& dsum, double& dsq) {
    constexpr int OH = Cfg::OH, PLANE = OH * OH * 8;
#pragma unroll
    for (int c = 0; c < CBW; ++c) {
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            float4 bv[4];
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) bv[rg] = *reinterpret_cast<const float4*>(s_bias + c * 32 + 8 * rg + 4 * h);
            const int oy = oy_w + Cfg::TILE_ROWS * i + prow, ox = ox0 + pcol;
            const bool valid = oy < OH && ox < OH;
            const int loff = (oy * OH + ox) * 8 + 4 * h;
            float fsum = 0.f, fsq = 0.f;
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                float4 v;
                v.x = fmaf(acc[c][i][4 * rg + 0], unscale, bv[rg].x);     // unscale = 2^-k exactly: one rounding, like acc + bias
                v.y = fmaf(acc[c][i][4 * rg + 1], unscale, bv[rg].y);
                v.z = fmaf(acc[c][i][4 * rg + 2], unscale, bv[rg].z);
                v.w = fmaf(acc[c][i][4 * rg + 3], unscale, bv[rg].w);
                if (valid) {
                    if (store) *reinterpret_cast<float4*>(out_blk + (loff + (c * 4 + rg) * PLANE)) = v;
                    fsum += (v.x + v.y) + (v.z + v.w);
                    fsq = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, fsq))));
                }
            }
            dsum += (double)fsum;
            dsq += (double)fsq;
        }
    }
}

// a wave's sums -> its slot (sum, sum of squares) of the workgroup's LDS array; a barrier later one thread adds the slots in
// wave order and writes the tile's partial moments
__device__ __forceinline__ void conv_wave_stats(double dsum, double dsq, int lane, double* slot) {
    const double lsum = wave_sum_d(dsum), lsq = wave_sum_d(dsq);
    if (lane == 0) { slot[0] = lsum; slot[1] = lsq; }
}
__device__ __forceinline__ void conv_publish_stats(const double* s_red, int nwaves, GNStats& o) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < nwaves; ++w) { a += s_red[2 * w]; b += s_red[2 * w + 1]; }
    o.sum = a;
    o.sq = b;
}
