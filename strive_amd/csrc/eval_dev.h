// Device functions shared by the evaluation metric kernels (eval_metrics.hip; dataset.hip includes it too): every formula that
// more than one metric needs is written here once, and so is every step that more than one kernel takes -- a scene's prologue
// (scene_span), the sampling grid (grid_ratios, sample_grid), the drivable test of a frame (road_samples, wave_off_road, off_road),
// the pair vote of a wave (wave_pair_vote), the rows of a grid (valid_frames, add_valid_rows), normalised inputs (EvalNorm) -- and
// the two argument checks the entry points share (eval_map_ok, eval_norm_fill).  The arithmetic helpers run under `#pragma clang fp contract(off)`: every operation is rounded on its
// own, so a formula gives the same bits whichever kernel asks for it, on the device and in a host build.  The box geometry is
// the exception: rect_iou_kernel reports its IoU, so it stays under the library's contraction rule as it always was; every
// other user only compares the IoU with EVAL_IOU_THRESH.
#pragma once
#include "common.h"
#include "crop_dev.h"

#define EVAL_IOU_THRESH 0.02                 // check_single_veh_coll / check_pairwise_veh_coll: a hit is IoU > 0.02
#define EVAL_NO_KEY 0x7fffffff               // a shared integer minimum that no (step, agent) key has entered
#define EVAL_NAN_BITS 0x7ff8000000000000ll
#define EVAL_DEG_PER_RAD (180.0 / 3.14159265358979323846)

__device__ __forceinline__ double eval_nan() { return __longlong_as_double(EVAL_NAN_BITS); }
__device__ __forceinline__ float eval_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double eval_sqrt(double v) { return sqrt(v); }

template <typename PoseT>
__device__ __forceinline__ bool nan4(const PoseT* p) { return p[0] != p[0] || p[1] != p[1] || p[2] != p[2] || p[3] != p[3]; }

// ---- rotated-box geometry: corners = R(atan2(hy, hx)) * (+-l/2, +-w/2) + (x, y) ----
template <typename PoseT>
__device__ __forceinline__ void box_corners(const PoseT* b, const float* lw, double cx[4], double cy[4]) {
    const double hl = 0.5 * (double)lw[0], hw = 0.5 * (double)lw[1];
    const double h = atan2((double)b[3], (double)b[2]);
    const double c = cos(h), s = sin(h);
    const double lx[4] = {-hl, hl, hl, -hl}, ly[4] = {-hw, -hw, hw, hw};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        cx[i] = lx[i] * c - ly[i] * s + (double)b[0];
        cy[i] = lx[i] * s + ly[i] * c + (double)b[1];
    }
}

__device__ __forceinline__ double poly_area(const double* x, const double* y, int n) {
    double a = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = (i + 1 == n) ? 0 : i + 1;
        a += x[i] * y[j] - x[j] * y[i];
    }
    return 0.5 * fabs(a);
}

// IoU of two counter-clockwise quadrilaterals: a is clipped against the four edges of b (Sutherland-Hodgman, <= 8 vertices)
__device__ __forceinline__ double quad_clip_iou(const double ax[4], const double ay[4], const double bx[4], const double by[4]) {
    double px[10], py[10], qx[10], qy[10];
    int n = 4;
    for (int i = 0; i < 4; ++i) { px[i] = ax[i]; py[i] = ay[i]; }
    // both quadrilaterals are counter-clockwise: "inside" of edge (e0 -> e1) is the left side
    for (int e = 0; e < 4 && n > 0; ++e) {
        const double ex = bx[e], ey = by[e];
        const double dx = bx[(e + 1) & 3] - ex, dy = by[(e + 1) & 3] - ey;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int j = (i + 1 == n) ? 0 : i + 1;
            const double si = dx * (py[i] - ey) - dy * (px[i] - ex);
            const double sj = dx * (py[j] - ey) - dy * (px[j] - ex);
            if (si >= 0.0) { qx[m] = px[i]; qy[m] = py[i]; ++m; }
            if ((si >= 0.0) != (sj >= 0.0)) {
                const double t = si / (si - sj);
                qx[m] = px[i] + t * (px[j] - px[i]);
                qy[m] = py[i] + t * (py[j] - py[i]);
                ++m;
            }
        }
        n = m;
        for (int i = 0; i < n; ++i) { px[i] = qx[i]; py[i] = qy[i]; }
    }
    const double inter = n >= 3 ? poly_area(px, py, n) : 0.0;
    const double uni = poly_area(ax, ay, 4) + poly_area(bx, by, 4) - inter;
    return inter / uni;
}

// IoU of the boxes of two poses; a NaN in either pose gives NaN
template <typename PA, typename PB>
__device__ __forceinline__ double box_iou(const PA* a, const float* lwa, const PB* b, const float* lwb) {
    double ax[4], ay[4], bx[4], by[4];
    box_corners(a, lwa, ax, ay);
    box_corners(b, lwb, bx, by);
    return quad_clip_iou(ax, ay, bx, by);
}

// the collision test of every metric: both poses hold no NaN (the reference skips such frames) and the boxes overlap
template <typename PA, typename PB>
__device__ __forceinline__ bool boxes_hit(const PA* a, const float* lwa, const PB* b, const float* lwb) {
    return !nan4(a) && !nan4(b) && box_iou(a, lwa, b, lwb) > EVAL_IOU_THRESH;
}

// A reject before the clip: the centres lie further apart than the two half-diagonals together, so the boxes share no point and
// their IoU is 0.  Exact as a decision on IoU > EVAL_IOU_THRESH: where rounding could turn this comparison the boxes touch at
// most at a corner.  false for a NaN anywhere (the clip decides).
template <typename PA, typename PB>
__device__ __forceinline__ bool boxes_apart(const PA* a, const float* lwa, const PB* b, const float* lwb) {
#pragma clang fp contract(off)
    const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1];
    const double la = (double)lwa[0], wa = (double)lwa[1], lb = (double)lwb[0], wb = (double)lwb[1];
    const double r = 0.5 * (sqrt(la * la + wa * wa) + sqrt(lb * lb + wb * wb));
    return dx * dx + dy * dy > r * r;
}

// One fine frame j of interp_traj (reference src/losses/adv_gen_nusc.py:625-644) of the trajectory tr (T, 4) up-sampled by
// 1 / rs: half-pixel linear taps as ATen's area_pixel_compute_source_index evaluates them in the tensor's type S, heading
// renormalised.  A NaN tap gives a NaN frame.
template <typename S>
__device__ __forceinline__ void fine_frame(const S* tr, int T, int j, S rs, S u[4]) {
#pragma clang fp contract(off)
    S src = rs * ((S)j + (S)0.5) - (S)0.5;
    src = src < (S)0 ? (S)0 : src;
    int i0 = (int)src;
    i0 = i0 > T - 1 ? T - 1 : i0;
    const int i1 = i0 < T - 1 ? i0 + 1 : i0;
    const S w1 = src - (S)i0, w0 = (S)1 - w1;
    for (int c = 0; c < 4; ++c) u[c] = w0 * tr[i0 * 4 + c] + w1 * tr[i1 * 4 + c];
    const S nrm = eval_sqrt(u[2] * u[2] + u[3] * u[3]);
    u[2] = u[2] / nrm;
    u[3] = u[3] / nrm;
}

// (sic) the coarse frame of a fine step, in the reference's order of operations: int((t_fine * (dt / scale)) / dt)
__device__ __forceinline__ int coarse_index(int fine_t, double dt, int scale) {
#pragma clang fp contract(off)
    const double interp_dt = dt / (double)scale;
    return (int)(((double)fine_t * interp_dt) / dt);
}

// speed of a relative to b at impact from the coarse frames (idx - 1, idx), frames (0, 1) for idx = 0
template <typename PA, typename PB>
__device__ __forceinline__ double rel_speed(const PA* a, const PB* b, int idx, double dt) {
#pragma clang fp contract(off)
    const int f1 = idx > 0 ? idx : 1, f0 = f1 - 1;
    const double rx = ((double)a[f1 * 4 + 0] - (double)a[f0 * 4 + 0]) / dt - ((double)b[f1 * 4 + 0] - (double)b[f0 * 4 + 0]) / dt;
    const double ry = ((double)a[f1 * 4 + 1] - (double)a[f0 * 4 + 1]) / dt - ((double)b[f1 * 4 + 1] - (double)b[f0 * 4 + 1]) / dt;
    return sqrt(rx * rx + ry * ry);
}

// compute_accels (reference src/eval_adv_gen.py:323-337, src/eval_planner.py:176-216) on the first m frames of one trajectory,
// frame 0 upwards: speeds along the unit headings, then sum and max of |accel|, of the forward and of the lateral acceleration
template <typename PoseT>
__device__ __forceinline__ void accel_series(const PoseT* tr, int m, double dt, double sum[3], double mx[3], int& cnt) {
#pragma clang fp contract(off)
    double s_prev = 0.0, vx_prev = 0.0, vy_prev = 0.0, lx_prev = 0.0, ly_prev = 0.0;
    for (int i = 0; i + 1 < m; ++i) {
        const double dx = ((double)tr[(i + 1) * 4 + 0] - (double)tr[i * 4 + 0]) / dt;
        const double dy = ((double)tr[(i + 1) * 4 + 1] - (double)tr[i * 4 + 1]) / dt;
        const double s = sqrt(dx * dx + dy * dy);
        const double hx = (double)tr[i * 4 + 2], hy = (double)tr[i * 4 + 3];
        const double hn = sqrt(hx * hx + hy * hy);
        const double ux = hx / hn, uy = hy / hn;
        const double vx = s * ux, vy = s * uy;
        if (i > 0) {
            const double fwd = fabs((s - s_prev) / dt);
            const double acx = (vx - vx_prev) / dt, acy = (vy - vy_prev) / dt;
            const double lat = fabs(acx * lx_prev + acy * ly_prev);
            const double acc = sqrt(acx * acx + acy * acy);
            const double v[3] = {acc, fwd, lat};
            for (int c = 0; c < 3; ++c) {
                sum[c] += v[c];
                mx[c] = (cnt == 0 || v[c] > mx[c] || v[c] != v[c]) ? v[c] : mx[c];
            }
            ++cnt;
        }
        s_prev = s; vx_prev = vx; vy_prev = vy;
        lx_prev = -uy; ly_prev = ux;
    }
}

// position error (m) and angle between the unit headings (radians, the dot product clamped to [-1, 1]) of two fp32 poses
__device__ __forceinline__ void pose_err(const float* g, const float* p, double& pos, double& rad) {
#pragma clang fp contract(off)
    const double ex = (double)g[0] - (double)p[0], ey = (double)g[1] - (double)p[1];
    pos = sqrt(ex * ex + ey * ey);
    const double gx = (double)g[2], gy = (double)g[3], qx = (double)p[2], qy = (double)p[3];
    const double gn = sqrt(gx * gx + gy * gy), qn = sqrt(qx * qx + qy * qy);
    double dot = (gx / gn) * (qx / qn) + (gy / gn) * (qy / qn);
    dot = dot < -1.0 ? -1.0 : (dot > 1.0 ? 1.0 : dot);
    rad = acos(dot);
}

// ---- drivable area (check_on_layer, reference src/datasets/nuscenes_utils.py:266-298) on raster layer 0 of map m ----
__device__ __forceinline__ CropFrame map_frame(const StriveMap& map, int m, const float* pose) {
    CropFrame fr;
    fr.x = pose[0]; fr.y = pose[1]; fr.hc = pose[2]; fr.hs = pose[3];
    set_crop_scale(fr, map.dx[m * 2 + 0], map.dx[m * 2 + 1]);
    fr.H = map.H;
    fr.W = map.W;
    fr.base = map.raster + (size_t)m * map.C * map.H * map.W;
    return fr;
}

// one coordinate of the sampling grid in the vehicle's frame: (linspace(-1, 1, k)[i] * size) / 2 in fp32
__device__ __forceinline__ float grid_coord(float lin, float size) { return __fmul_rn(lin, size) * 0.5f; }

// is the grid sample (lwise, wwise) of the frame on the road (fp64 divide, round half even, out of bounds -> pixel (0,0))
__device__ __forceinline__ int on_road(const CropFrame& fr, float lwise, float wwise) {
    int px, py;
    float gx, gy;
    crop_world(fr, lwise, wwise, gx, gy);
    world_to_pixel(fr, gx, gy, px, py);
    return fr.base[(size_t)py * fr.W + px] != 0 ? 1 : 0;
}

// row k of the caller's linspace table: fp32 linspace(-1, 1, k) for k = 1, 2, ... one after the other, so row k starts at
// k (k - 1) / 2.  k <= 0 (no grid) gives the table's start, of which nothing is read.
__device__ __forceinline__ const float* lin_row(const float* lin_tab, int k) { return lin_tab + (k > 0 ? (size_t)k * (k - 1) / 2 : 0); }

// the drivable test of one frame: `on` of its `cells` grid samples lie on the road; off road is fp32(on) / fp32(cells) < fp32(1 - 0.05)
__device__ __forceinline__ bool off_road(int on, int cells) { return __fdiv_rn((float)on, (float)cells) < (float)(1.0 - 0.05); }

// road_samples: how many of the samples first, first + stride, ... of the L x W grid (L, W >= 1; sample c: row c / W, column c % W) of the
// frame `pose` (no NaN) of a vehicle of size lw lie on the road of map m.  Integer counts: the order of the samples does not matter.
// (Row and column are carried from sample to sample -- a stride is di rows and dj < W columns -- so the loop holds no division.)
__device__ __forceinline__ int road_samples(const StriveMap& map, int m, const float* pose, const float* lw, const float* lin_tab,
                                            int L, int W, int first, int stride) {
    const CropFrame fr = map_frame(map, m, pose);
    const float* lin_l = lin_row(lin_tab, L);
    const float* lin_w = lin_row(lin_tab, W);
    const int di = stride / W, dj = stride - di * W;
    int i = first / W, j = first - i * W, on = 0;
    for (int c = first; c < L * W; c += stride) {
        on += on_road(fr, grid_coord(lin_l[i], lw[0]), grid_coord(lin_w[j], lw[1]));
        i += di;
        j += dj;
        if (j >= W) {
            j -= W;
            ++i;
        }
    }
    return on;
}

// wave_off_road: the drivable test of one frame by ONE WAVE: its lanes stride over the samples (road_samples) and add their counts,
// so every lane returns the same answer (L, W >= 1).
__device__ __forceinline__ bool wave_off_road(const StriveMap& map, int m, const float* pose, const float* lw, const float* lin_tab,
                                              int L, int W, int lane) {
    int on = road_samples(map, m, pose, lw, lin_tab, L, W, lane, 64);
    for (int k = 32; k >= 1; k >>= 1) on += __shfl_xor(on, k);
    return off_road(on, L * W);
}

// Sampling grid of check_on_layer from `rows` valid rows with the sums sl, sw of their vehicle sizes: the mean size and its
// ratio to mean(dx) over all entries of the map's dx, length then width (L = rint(ratio[0]), W likewise: sample_grid below, or
// the caller's own rule).  false, and nothing written, without a valid row.
__device__ __forceinline__ bool grid_ratios(long long rows, double sl, double sw, const StriveMap& map, double mean[2], double ratio[2]) {
#pragma clang fp contract(off)
    if (rows <= 0) return false;
    double sdx = 0.0;
    for (int m = 0; m < map.M * 2; ++m) sdx += map.dx[m];
    const double mdx = sdx / (double)(map.M * 2);
    mean[0] = sl / (double)rows;
    mean[1] = sw / (double)rows;
    ratio[0] = mean[0] / mdx;
    ratio[1] = mean[1] / mdx;
    return true;
}

// sample_grid: L and W of the sampling grid on top of grid_ratios, as the kernels that serve ONE call of check_on_layer form it:
// rint of the two ratios, each inside what the caller's linspace table holds (1..lin_max).  Without a valid row there is no grid:
// L = W = 0, mean and ratio untouched, true.  false: an axis is outside the table (its size is then -1) and the caller refuses
// the scene with status 4.
__device__ __forceinline__ bool sample_grid(long long rows, double sl, double sw, const StriveMap& map, int lin_max, double mean[2],
                                            double ratio[2], int& L, int& W) {
    L = W = 0;
    if (!grid_ratios(rows, sl, sw, map, mean, ratio)) return true;
    const double ql = rint(ratio[0]), qw = rint(ratio[1]);
    L = (ql >= 1.0 && ql <= (double)lin_max) ? (int)ql : -1;
    W = (qw >= 1.0 && qw <= (double)lin_max) ? (int)qw : -1;
    return L > 0 && W > 0;
}

// ---- normalised inputs: the statistics of the two MeanStdNormalizers, and v * std + mean in fp32 (unnorm1) as the reference's
// unnormalize forms it ----
struct EvalNorm { float sm[4], ss[4], am[2], asd[2]; };     // state mean / std (x, y, hcos, hsin), attribute mean / std (l, w)

__device__ __forceinline__ void unnorm_pose(const EvalNorm& N, const float* p, float u[4]) {
    for (int c = 0; c < 4; ++c) u[c] = unnorm1(p[c], N.sm[c], N.ss[c]);
}

// the size of agent ag of the normalised sizes lw (., 2)
__device__ __forceinline__ void unnorm_lw(const EvalNorm& N, const float* lw, int ag, float u[2]) {
    u[0] = unnorm1(lw[(size_t)ag * 2 + 0], N.am[0], N.asd[0]);
    u[1] = unnorm1(lw[(size_t)ag * 2 + 1], N.am[1], N.asd[1]);
}

// valid_frames: how many of the `frames` poses of tr hold no NaN after unnormalising (the rows check_on_layer keeps)
__device__ __forceinline__ int valid_frames(const EvalNorm& N, const float* tr, size_t frames) {
    int c = 0;
    for (size_t f = 0; f < frames; ++f) {
        float u[4];
        unnorm_pose(N, tr + f * 4, u);
        c += nan4(u) ? 0 : 1;
    }
    return c;
}

// add_valid_rows: agent ag with the trajectory tr enters a grid's row count and size sums with count * size (not at all without
// a valid frame: its size may be anything)
__device__ __forceinline__ void add_valid_rows(const EvalNorm& N, const float* tr, size_t frames, const float* lw, int ag,
                                               long long& cnt, double& sl, double& sw) {
#pragma clang fp contract(off)
    const int c = valid_frames(N, tr, frames);
    if (c <= 0) return;
    float lwu[2];
    unnorm_lw(N, lw, ag, lwu);
    cnt += c;
    sl += (double)c * (double)lwu[0];
    sw += (double)c * (double)lwu[1];
}

// ---- the prologue of a scene: its agents and whether the kernel may touch them ----
__device__ __forceinline__ bool map_index_ok(int m, int M) { return m >= 0 && m < M; }      // M: the map set's StriveMap.M

// scene_span: the agents [a0, a0 + n) of scene b from the offsets ptr (B+1) and the scene's status: 2 when they leave the NA rows
// or n < 1 (nothing of the scene may be read), else, where the kernel asks for a map (mapix given), map_code for a map index
// outside the M maps, else 0.  Uniform over the workgroup.
__device__ __forceinline__ int scene_span(const int32_t* ptr, int b, int NA, int& a0, int& n, const int32_t* mapix = nullptr,
                                          int M = 0, int map_code = 0) {
    a0 = ptr[b];
    const int a1 = ptr[b + 1];
    n = a1 - a0;
    if (a0 < 0 || n <= 0 || a1 > NA) return 2;
    if (mapix && !map_index_ok(mapix[b], M)) return map_code;
    return 0;
}

// wave_pair_vote: one agent against the agents that follow it, by ONE WAVE.  pi (T,4) is the agent's trajectory and lwi its
// unnormalised size; the other agents' trajectories start at pj, jstride floats apart, their normalised sizes at lwj.  The lanes
// stride over the items e = dj * T + t (other agent dj, step t), test the two boxes of the step (REJECT: boxes_apart first, which
// decides the same and spares the clip; then boxes_hit, for which a frame with a NaN is no hit) and vote.  Returns the lowest
// hitting item of the first 64 that hold one -- for a single other agent the first step of contact -- or `items` without a hit; the
// same value in every lane.
template <bool REJECT>
__device__ __forceinline__ int wave_pair_vote(const EvalNorm& N, const float* pi, const float* lwi, const float* pj, size_t jstride,
                                              const float* lwj, int items, int T, int lane) {
    for (int base = 0; base < items; base += 64) {
        const int e = base + lane;
        bool h = false;
        if (e < items) {
            const int dj = e / T, t = e - dj * T;
            float u[4], v[4], lwv[2];
            unnorm_pose(N, pi + (size_t)t * 4, u);
            unnorm_pose(N, pj + (size_t)dj * jstride + (size_t)t * 4, v);
            unnorm_lw(N, lwj, dj, lwv);
            h = !(REJECT && boxes_apart(u, lwi, v, lwv)) && boxes_hit(u, lwi, v, lwv);
        }
        const unsigned long long m = __ballot(h ? 1 : 0);
        if (m != 0ull) return base + __ffsll((long long)m) - 1;
    }
    return items;
}

// ---- host side: the argument checks the entry points share ----
static inline bool eval_map_ok(const StriveMap* map) {
    return map && map->raster && map->dx && map->M >= 1 && map->C >= 1 && map->H >= 1 && map->W >= 1;
}

// the normaliser statistics from the entry point's four host pointers; false, and nothing written, if one is missing
static inline bool eval_norm_fill(EvalNorm& N, const float* state_mean4, const float* state_std4, const float* att_mean2,
                                  const float* att_std2) {
    if (!state_mean4 || !state_std4 || !att_mean2 || !att_std2) return false;
    for (int c = 0; c < 4; ++c) {
        N.sm[c] = state_mean4[c];
        N.ss[c] = state_std4[c];
    }
    for (int c = 0; c < 2; ++c) {
        N.am[c] = att_mean2[c];
        N.asd[c] = att_std2[c];
    }
    return true;
}
