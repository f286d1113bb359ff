// Scene dataset: post-processing of track records into per-agent state tables, the agent counts of every window and the
// assembly of a batch of windows (reference src/datasets/nuscenes_dataset.py:416-589, :594-704, and the PyG DataLoader collation).
// float64 code on the helpers of eval_dev.h; every + - * / sqrt is rounded on its own (no contraction), so the tables carry the
// bits numpy gives the reference.
#include "eval_dev.h"

#pragma clang fp contract(off)

#define DS_NT 256
#define DS_TWO_PI 6.283185307179586          // 2 * np.pi
#define DS_PI 3.141592653589793              // np.pi

__device__ __forceinline__ bool ds_nan(double v) { return v != v; }
__device__ __forceinline__ bool ds_nan2(const double* p) { const double s = p[0] + p[1]; return s != s; }     // isnan(np.sum(pos, axis=1))

// numpy's float remainder (npy_divmod): the result takes the sign of the divisor
__device__ __forceinline__ double ds_pymod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m = m + b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

// angle_diff (reference src/datasets/nuscenes_utils.py:134-143)
__device__ __forceinline__ double ds_angle_diff(double t1, double t2) {
    const double period = DS_TWO_PI, half = DS_TWO_PI / 2.0;
    double d = ds_pymod((t1 - t2) + half, period) - half;
    if (d > DS_PI) d = d - DS_TWO_PI;
    return d;
}

// velocity / heading_change_rate (:145-199): frame t takes the difference quotient k -> k + 1 with k = t - 1 (backward), k = 0 at
// frame 0 and k = t (forward) at a frame that follows a NaN frame -- unless that frame is the last one, which keeps its (NaN)
// backward difference.
__device__ __forceinline__ int ds_diff_index(int t, int T, bool nan_prev, bool nan_here) {
    if (t == 0) return 0;
    if (t < T - 1 && nan_prev && !nan_here) return t;
    return t - 1;
}

__device__ __forceinline__ double ds_time(const int64_t* ego_t, int t) { return (double)ego_t[t] * 1e-6; }

// pixel of one sample of check_on_layer's grid: float64 throughout, the division by dx as world_to_pixel predicts it
__device__ __forceinline__ size_t ds_sample_pixel(const double* ob, double lwise, double wwise, double dx0, double dx1, double inv0,
                                                  double inv1, int H, int W) {
    const double hc = ob[3], hs = ob[4];
    const double gx = (lwise * hc - wwise * hs) + ob[0];
    const double gy = (lwise * hs + wwise * hc) + ob[1];
    const double qx = quotient_rint(gx, dx0, inv0), qy = quotient_rint(gy, dx1, inv1);
    const bool inside = (qx == qx) & (qy == qy) & (qx >= 0.0) & (qx < (double)W) & (qy >= 0.0) & (qy < (double)H);
    const int px = inside ? (int)qx : 0, py = inside ? (int)qy : 0;
    return (size_t)py * W + px;
}

__global__ __launch_bounds__(DS_NT) void dataset_post_process_kernel(StriveTracks tr, StriveMap map, StriveSceneTables tb, int carpark,
                                                                       double mdx, const int32_t* __restrict__ lin_off,
                                                                       const float* __restrict__ lin, int nmax, double* __restrict__ ws) {
    __shared__ int s_any;
    const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = DS_NT >> 6;
    const int sc = tr.agent_scene[a];
    const int f0 = tr.frame_ptr[sc], T = tr.frame_ptr[sc + 1] - f0;
    const int64_t r0 = tb.row_ptr[a];
    double* cur = ws + r0 * 8;               // (T,5) x, y, hcos, hsin, h on the scene's timeline
    double* vel = cur + (size_t)T * 5;       // (T,2)
    double* hd = vel + (size_t)T * 2;        // (T)
    const bool ego = a == tr.agent_ptr[sc];
    const bool use = ego || tr.use[a] != 0;
    const int o0 = tr.obs_ptr[a], no = tr.obs_ptr[a + 1] - o0;
    const int64_t* ego_t = tr.ego_t + f0;
    if (tid == 0) s_any = 0;
    for (int i = tid; i < T * 5; i += DS_NT) cur[i] = eval_nan();
    __syncthreads();

    // ---- valid frames + scatter: one wave per observation, the lanes walk the sampling grid ----
    const double l = tr.lw[a * 2 + 0], w = tr.lw[a * 2 + 1];
    int L = 0, W = 0;
    bool grid_ok = true;
    if (!ego) {
        // (the reference rounds mean(lw rows) / mdx; the mean of n identical rows is l unless the n-fold float64 sum rounds: DESIGN 4.13e)
        const double rl = rint(l / mdx), rw = rint(w / mdx);
        grid_ok = rl >= 0.0 && rl <= (double)nmax && rw >= 0.0 && rw <= (double)nmax;
        L = grid_ok ? (int)rl : 0;
        W = grid_ok ? (int)rw : 0;
    }
    if (use && grid_ok) {
        const int m = tr.scene_map[sc];
        const bool map_ok = m >= 0 && m < map.M;
        const double dx0 = map_ok ? map.dx[m * 2 + 0] : 1.0, dx1 = map_ok ? map.dx[m * 2 + 1] : 1.0;
        const double inv0 = __ddiv_rn(1.0, dx0), inv1 = __ddiv_rn(1.0, dx1);
        const uint8_t* driv = map.raster + (size_t)(map_ok ? m : 0) * map.C * map.H * map.W;
        const uint8_t* park = driv + (size_t)(carpark > 0 ? carpark : 0) * map.H * map.W;
        const float* linl = lin + lin_off[L];
        const float* linw = lin + lin_off[W];
        const int LW = L * W;
        for (int k = wave; k < no; k += nw) {
            const double* ob = tr.obs + (size_t)(o0 + k) * 5;
            bool keep = ego || map_ok;
            if (!ego && map_ok) {
                int cd = 0, cp = 0;
                for (int s0 = 0; s0 < LW; s0 += 64) {
                    const int s = s0 + lane;
                    int on_d = 0, on_p = 0;
                    if (s < LW) {
                        const int i = s / W, j = s - i * W;
                        const double lwise = ((double)linl[i] * l) / 2.0, wwise = ((double)linw[j] * w) / 2.0;
                        const size_t pix = ds_sample_pixel(ob, lwise, wwise, dx0, dx1, inv0, inv1, map.H, map.W);
                        on_d = driv[pix] != 0;
                        on_p = carpark > 0 ? (park[pix] != 0) : 0;
                    }
                    cd += __builtin_popcountll(__ballot(on_d));
                    cp += __builtin_popcountll(__ballot(on_p));
                }
                const float den = (float)LW;
                const float fd = (float)cd / den, fp = (float)cp / den;
                keep = fd >= 0.3f && (carpark <= 0 || fp < 0.3f);
            }
            const int f = tr.obs_frame[o0 + k];
            if (keep && lane == 0 && f >= 0 && f < T) {
                double* c = cur + (size_t)f * 5;
                c[0] = ob[0]; c[1] = ob[1]; c[2] = ob[3]; c[3] = ob[4]; c[4] = ob[2];
                atomicOr(&s_any, 1);
            }
        }
    }
    __syncthreads();

    // ---- first differences ----
    for (int t = tid; t < T; t += DS_NT) {
        double vx = eval_nan(), vy = eval_nan(), hdot = eval_nan();
        if (T >= 2) {
            const double* p = cur + (size_t)t * 5;
            const int k = ds_diff_index(t, T, t > 0 && ds_nan2(p - 5), ds_nan2(p));
            const int kh = ds_diff_index(t, T, t > 0 && ds_nan(p[-1]), ds_nan(p[4]));
            const double* p0 = cur + (size_t)k * 5;
            const double dts = ds_time(ego_t, k + 1) - ds_time(ego_t, k);
            vx = (p0[5] - p0[0]) / dts;
            vy = (p0[6] - p0[1]) / dts;
            const double* h0 = cur + (size_t)kh * 5;
            hdot = ds_angle_diff(h0[9], h0[4]) / (ds_time(ego_t, kh + 1) - ds_time(ego_t, kh));
        }
        vel[t * 2 + 0] = vx;
        vel[t * 2 + 1] = vy;
        hd[t] = hdot;
    }
    __syncthreads();

    // ---- speeds, second differences, the tables ----
    const bool kept = use && (ego || s_any != 0);
    if (tid == 0) tb.kept[a] = kept ? 1 : 0;
    for (int t = tid; t < T; t += DS_NT) {
        const double vx = vel[t * 2 + 0], vy = vel[t * 2 + 1];
        const double s = sqrt(vx * vx + vy * vy);
        double acc = eval_nan(), ddh = eval_nan();
        if (T >= 2) {
            const int k = ds_diff_index(t, T, t > 0 && ds_nan2(vel + (t - 1) * 2), ds_nan2(vel + t * 2));
            const double dts = ds_time(ego_t, k + 1) - ds_time(ego_t, k);
            const double ax = (vel[(k + 1) * 2 + 0] - vel[k * 2 + 0]) / dts, ay = (vel[(k + 1) * 2 + 1] - vel[k * 2 + 1]) / dts;
            acc = sqrt(ax * ax + ay * ay);
            const int kh = ds_diff_index(t, T, t > 0 && ds_nan(hd[t - 1]), ds_nan(hd[t]));
            ddh = ds_angle_diff(hd[kh + 1], hd[kh]) / (ds_time(ego_t, kh + 1) - ds_time(ego_t, kh));
        }
        const bool no_vis = ds_nan(s);
        double* row = tb.traj + (size_t)(r0 + t) * 6;
        const double* c = cur + (size_t)t * 5;
        for (int q = 0; q < 4; ++q) row[q] = no_vis ? eval_nan() : c[q];
        row[4] = s;
        row[5] = hd[t];
        tb.accel[(size_t)(r0 + t) * 2 + 0] = acc;
        tb.accel[(size_t)(r0 + t) * 2 + 1] = ddh;
        tb.is_vis[r0 + t] = no_vis ? 0 : 1;
    }
}

extern "C" int strive_dataset_post_process(const StriveTracks* tr, const StriveMap* map, const StriveSceneTables* tb,
                                           int32_t carpark_layer, double mdx, const int32_t* lin_off, const float* lin, int32_t nmax,
                                           void* ws, size_t ws_bytes, strive_stream_t stream) {
    STRIVE_CHECK_ARG(tr && map && tb && lin_off && lin && ws, "null argument");
    STRIVE_CHECK_ARG(tr->A <= tb->A && tr->S <= tb->S, "more track agents or scenes than the tables hold");
    STRIVE_CHECK_ARG(tr->frame_ptr && tr->ego_t && tr->agent_ptr && tr->scene_map && tr->agent_scene && tr->use && tr->lw && tr->obs_ptr &&
                     tr->obs_frame && tr->obs, "null track array");
    STRIVE_CHECK_ARG(tb->row_ptr && tb->traj && tb->accel && tb->is_vis && tb->kept, "null table");
    STRIVE_CHECK_ARG(map->raster && map->dx && map->M > 0, "null map");
    STRIVE_CHECK_ARG(carpark_layer < map->C, "carpark layer outside the raster");
    STRIVE_CHECK_ARG(mdx > 0.0 && nmax >= 0, "bad grid scale");
    STRIVE_CHECK_ARG(ws_bytes >= (size_t)tb->R * 8 * sizeof(double), "workspace too small");
    if (tr->A <= 0) return 0;
    hipLaunchKernelGGL(dataset_post_process_kernel, dim3(tr->A), dim3(DS_NT), 0, (hipStream_t)stream, *tr, *map, *tb, (int)carpark_layer, mdx,
                       lin_off, lin, (int)nmax, (double*)ws);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// ---- agent selection of __getitem__ (:630-649) ----
__device__ __forceinline__ bool ds_row_has_nan(const double* row) {
    return ds_nan(row[0]) || ds_nan(row[1]) || ds_nan(row[2]) || ds_nan(row[3]) || ds_nan(row[4]) || ds_nan(row[5]);
}

__device__ __forceinline__ bool ds_selected(const StriveSceneTables& tb, int a, bool ego, int midx, int full_past) {
    if (ego) return true;
    if (!tb.kept[a]) return false;
    const double* tj = tb.traj + (size_t)tb.row_ptr[a] * 6;
    if (ds_row_has_nan(tj + (size_t)(midx - 1) * 6)) return false;
    if (full_past)
        for (int r = 0; r < midx; ++r)           // (sic) traj[:midx]: from the scene's first frame, not the window's
            if (ds_row_has_nan(tj + (size_t)r * 6)) return false;
    return true;
}

// a window lies in its scene's tables
__device__ __forceinline__ bool ds_window_ok(const StriveSceneTables& tb, int sc, int sidx, int npast, int nfuture) {
    return sc >= 0 && sc < tb.S && sidx >= 0 && npast >= 1 && sidx + npast + nfuture <= tb.scene_T[sc];
}

__global__ __launch_bounds__(64) void dataset_window_counts_kernel(StriveSceneTables tb, const int32_t* __restrict__ seq, int npast,
                                                                     int nfuture, int full_past, int32_t* __restrict__ counts) {
    const int wi = blockIdx.x, lane = threadIdx.x;
    const int sc = seq[wi * 2 + 0], sidx = seq[wi * 2 + 1];
    if (!ds_window_ok(tb, sc, sidx, npast, nfuture)) {
        if (lane == 0) counts[wi] = 0;
        return;
    }
    const int a0 = tb.agent_ptr[sc], n = tb.agent_ptr[sc + 1] - a0, midx = sidx + npast;
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const int sel = j < n && ds_selected(tb, a0 + j, j == 0, midx, full_past);
        cnt += __builtin_popcountll(__ballot(sel));
    }
    if (lane == 0) counts[wi] = cnt;
}

extern "C" int strive_dataset_window_counts(const StriveSceneTables* tb, const int32_t* seq, int32_t N, int32_t npast, int32_t nfuture,
                                            int32_t require_full_past, int32_t* counts, strive_stream_t stream) {
    STRIVE_CHECK_ARG(tb && seq && counts, "null argument");
    STRIVE_CHECK_ARG(tb->agent_ptr && tb->scene_T && tb->row_ptr && tb->traj && tb->kept, "null table");
    STRIVE_CHECK_ARG(npast >= 1 && nfuture >= 0, "bad window");
    if (N <= 0) return 0;
    hipLaunchKernelGGL(dataset_window_counts_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, *tb, seq, (int)npast, (int)nfuture,
                       (int)require_full_past, counts);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// ---- batch assembly ----
struct DatasetBatchOut {
    float *past, *past_gt, *future, *future_gt, *lw, *sem, *past_vis, *future_vis;
    int64_t *batch, *map_idx, *edge_index;
    int64_t E;
};

// rows [first, first + n) of agent a as n normalised fp32 states (torch.Tensor(float64 array), then (x - mean) / std in fp32)
__device__ __forceinline__ void ds_copy_states(const StriveSceneTables& tb, int a, int first, int n, const StriveNorm& nm, float* out,
                                               float* out_gt, float* vis) {
    const int64_t r0 = tb.row_ptr[a] + first;
    for (int r = 0; r < n; ++r) {
        const double* row = tb.traj + (size_t)(r0 + r) * 6;
        for (int c = 0; c < 6; ++c) {
            const float v = norm1((float)row[c], nm.state_mean[c], nm.state_std[c]);
            out[r * 6 + c] = v;
            out_gt[r * 6 + c] = v;
        }
        vis[r] = (float)tb.is_vis[r0 + r];
    }
}

__global__ __launch_bounds__(DS_NT) void dataset_gather_kernel(StriveSceneTables tb, const int32_t* __restrict__ seq,
                                                                 const int64_t* __restrict__ meta, int B, int npast, int nfuture, int NC,
                                                                 int full_past, StriveNorm nm, DatasetBatchOut o) {
    __shared__ int s_wave[DS_NT / 64];
    __shared__ int s_base;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t wi = meta[b];
    const int64_t node0 = meta[(B + 1) + b], nsel = meta[(B + 1) + b + 1] - node0, e0 = meta[2 * (B + 1) + b];
    const int sc = seq[wi * 2 + 0], sidx = seq[wi * 2 + 1], midx = sidx + npast;
    if (!ds_window_ok(tb, sc, sidx, npast, nfuture)) return;
    const int a0 = tb.agent_ptr[sc], n = tb.agent_ptr[sc + 1] - a0;
    if (tid == 0) {
        s_base = 0;
        o.map_idx[b] = tb.scene_map[sc];
    }
    __syncthreads();
    // ordered compaction of the selected agents: ranks inside a wave from its ballot, the waves' totals through shared memory, the
    // running total of earlier passes in s_base (a scene may hold more agents than the workgroup has threads)
    for (int j0 = 0; j0 < n; j0 += DS_NT) {
        const int j = j0 + tid;
        const int sel = j < n && ds_selected(tb, a0 + j, j == 0, midx, full_past);
        const unsigned long long mask = __ballot(sel);
        const int rank = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __builtin_popcountll(mask);
        __syncthreads();
        int off = s_base;
        for (int v = 0; v < wave; ++v) off += s_wave[v];
        const int64_t slot = off + rank;
        if (sel && slot < nsel) {
            const int a = a0 + j;
            const int64_t node = node0 + slot;
            ds_copy_states(tb, a, sidx, npast, nm, o.past + node * npast * 6, o.past_gt + node * npast * 6, o.past_vis + node * npast);
            ds_copy_states(tb, a, midx, nfuture, nm, o.future + node * nfuture * 6, o.future_gt + node * nfuture * 6,
                           o.future_vis + node * nfuture);
            for (int c = 0; c < 2; ++c) o.lw[node * 2 + c] = norm1((float)tb.lw[a * 2 + c], nm.att_mean[c], nm.att_std[c]);
            const int cat = tb.cat[a];
            for (int c = 0; c < NC; ++c) o.sem[node * NC + c] = c == cat ? 1.0f : 0.0f;
            o.batch[node] = b;
        }
        __syncthreads();
        if (tid == 0) {
            int tot = s_base;
            for (int v = 0; v < DS_NT / 64; ++v) tot += s_wave[v];
            s_base = tot;
        }
        __syncthreads();
    }
    // the source-major clique without self loops, offset by the window's first node
    const int64_t ne = nsel * (nsel - 1);
    for (int64_t e = tid; e < ne; e += DS_NT) {
        const int64_t i = e / (nsel - 1), r = e - i * (nsel - 1);
        const int64_t j = r + (r >= i ? 1 : 0);
        o.edge_index[e0 + e] = node0 + i;
        o.edge_index[o.E + e0 + e] = node0 + j;
    }
}

extern "C" int strive_dataset_gather_batch(const StriveSceneTables* tb, const int32_t* seq, const int64_t* meta, int32_t B, int32_t npast,
                                           int32_t nfuture, int32_t NC, int32_t require_full_past, const StriveNorm* norm, float* past,
                                           float* past_gt, float* future, float* future_gt, float* lw, float* sem, float* past_vis,
                                           float* future_vis, int64_t* batch, int64_t* map_idx, int64_t* edge_index, int64_t E,
                                           strive_stream_t stream) {
    STRIVE_CHECK_ARG(tb && seq && meta && norm && map_idx, "null argument");
    STRIVE_CHECK_ARG(past && past_gt && future && future_gt && lw && sem && past_vis && future_vis && batch, "null output");
    STRIVE_CHECK_ARG(edge_index || E == 0, "null edge_index");
    STRIVE_CHECK_ARG(tb->agent_ptr && tb->scene_T && tb->scene_map && tb->row_ptr && tb->cat && tb->lw && tb->traj && tb->is_vis && tb->kept,
                     "null table");
    STRIVE_CHECK_ARG(npast >= 1 && nfuture >= 0 && NC >= 1 && E >= 0, "bad window");
    if (B <= 0) return 0;
    DatasetBatchOut o = {past, past_gt, future, future_gt, lw, sem, past_vis, future_vis, batch, map_idx, edge_index, E};
    hipLaunchKernelGGL(dataset_gather_kernel, dim3(B), dim3(DS_NT), 0, (hipStream_t)stream, *tb, seq, meta, (int)B, (int)npast, (int)nfuture,
                       (int)NC, (int)require_full_past, *norm, o);
    STRIVE_CHECK_LAUNCH();
    return 0;
}
