// Draw tables of a live batch, built where the batch is: what viz_scene_graph hands to viz_map_crop / viz_map_crop_video and the
// artists render_obj_observation makes of it, as the tables strive_render_pictures reads.
// (reference src/datasets/nuscenes_utils.py:477-621 viz_scene_graph, :632-653 viz_map_crop_video, :733-835
//  render_obj_observation; src/datasets/map_env.py:231-254 objs2crop)
//
// The contract -- frame, order of the records, NaN rule, centroid rule, status bits -- is the text above StriveSceneDraw in
// include/strive_hip.h.
//
// Work decomposition: a workgroup of 256 threads owns one picture (grid-stride over the pictures).  A picture's candidate
// items -- steps, trajectories, agents, each in the reference's loop order -- are walked in passes of 256, thread i of a pass
// evaluating item i; a workgroup scan of the "is drawn" flags (shuffles inside a wave, the four wave totals through LDS) gives
// every drawn item its place in the picture's slot, so the slot is filled densely, in order, without atomics.  A step's crop
// values are recomputed where a later pass needs them (a trajectory's count, the initial car) instead of being kept: a step is
// four loads and a few transcendental calls, and nothing is stored between the passes but the running totals.
#include "common.h"

#pragma clang fp contract(off)

namespace {
constexpr int SD_THREADS = 256;
constexpr int RPF = STRIVE_RENDER_PRIM_FLOATS;
constexpr int VI = STRIVE_SCENE_DRAW_VIEW_INTS;
constexpr int PI = STRIVE_SCENE_DRAW_PIC_INTS;

struct Lds {
    double sx[SD_THREADS], sy[SD_THREADS];
    int cnt[SD_THREADS];
    int wave[SD_THREADS / 64];
    float pose[4];
};

// what a picture draws, resolved from its view and picture records; uniform over the workgroup
struct Pic {
    int a0, n;                          // the scene's first agent and size
    int d_src, d_cnt, g_src, g_cnt;     // drawn agents, ground-truth agents (scene-local)
    int NS, FPT;                        // of the drawn future
    int s0, ns, t0, nt;                 // the window of samples and steps this picture shows
    int gNT;                            // steps of a ground-truth trajectory
    int rb, rb_gt, style;               // first rows of the colour tables, -1: default styles
    bool traj, ow;
    const float* fut;                   // the drawn future: (agent, sample, step) strides below
    long long fa, fs, ft;
    float b0, b1, sl, sw;
};

// exclusive scan of v over the workgroup in thread order; total = the sum.  Every thread calls it.
__device__ __forceinline__ int block_exscan(int v, int* s_wave, int& total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                     // the previous scan's totals have been read
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int i = 0; i < SD_THREADS / 64; ++i) {
        if (i < w) base += s_wave[i];
        total += s_wave[i];
    }
    return base + inc - v;
}

__device__ __forceinline__ bool is_nan(float v) { return !(v == v); }

// the unnormalised state (x, y, hx, hy) of step t of a trajectory whose first PT steps are the agent's past
__device__ __forceinline__ void load_step(const StriveSceneDraw& J, int agent, int t, const float* fut, long long fut_off, long long ft,
                                          float o[4]) {
    const float* src = t < J.PT ? J.past_gt + ((long long)agent * J.PT + t) * J.past_stride : fut + fut_off + (long long)(t - J.PT) * ft;
    for (int c = 0; c < 4; ++c) o[c] = unnorm1(src[c], J.norm.state_mean[c], J.norm.state_std[c]);
}

// objs2crop of one object; -> no NaN among the four values
__device__ __forceinline__ bool to_crop(const Pic& P, const float* pose, const float in[4], float o[4]) {
    const float theta = atan2f(pose[3], pose[2]);
    const float c = cosf(theta), s = sinf(theta);
    const float dx = in[0] - pose[0], dy = in[1] - pose[1];
    const float lx = dx * c + dy * s, ly = dy * c - dx * s;
    const float nh = atan2f(in[3], in[2]) - theta;
    o[0] = (lx - P.b0) * P.sl;
    o[1] = (ly - P.b1) * P.sw;
    o[2] = cosf(nh);
    o[3] = sinf(nh);
    return !(is_nan(o[0]) || is_nan(o[1]) || is_nan(o[2]) || is_nan(o[3]));
}

// step t (window-local) of sample s (window-local) of drawn agent j
__device__ __forceinline__ bool pred_step(const StriveSceneDraw& J, const Pic& P, const float* pose, int j, int s, int t, float o[4]) {
    const int agent = P.a0 + P.d_src + j;
    float in[4];
    load_step(J, agent, P.t0 + t, P.fut, (long long)agent * P.fa + (long long)(P.s0 + s) * P.fs, P.ft, in);
    return to_crop(P, pose, in, o);
}

// step t of ground-truth agent j
__device__ __forceinline__ bool gt_step(const StriveSceneDraw& J, const Pic& P, const float* pose, int j, int t, float o[4]) {
    const int agent = P.a0 + P.g_src + j;
    float in[4];
    if (P.ow) load_step(J, agent, t, J.ow_gt, (long long)agent * J.FT * 4, 4, in);
    else load_step(J, agent, t, J.future_gt, (long long)agent * J.FT * J.future_stride, J.future_stride, in);
    return to_crop(P, pose, in, o);
}

struct Style { float r, g, b, alpha, width, size; };

__device__ __forceinline__ Style style_of(const StriveSceneDraw& J, const Pic& P, int j) {
    Style st;
    if (P.style >= 0) {
        const float* s = J.style + (long long)(P.style + j) * 8;
        st.r = s[0]; st.g = s[1]; st.b = s[2]; st.alpha = s[3]; st.width = s[4]; st.size = s[5];
    } else {
        const float* c = J.cycle_rgb + (j % 9) * 3;
        st.r = c[0]; st.g = c[1]; st.b = c[2]; st.alpha = 0.7f; st.width = 1.0f; st.size = 8.0f;
    }
    return st;
}

__device__ __forceinline__ Style gt_style() {
    Style st;
    st.r = 1.0f; st.g = 1.0f; st.b = 1.0f; st.alpha = 0.7f; st.width = 1.0f; st.size = 8.0f;
    return st;
}

__device__ __forceinline__ void store_rec(float* dst, int kind, float cx, float cy, float hx, float hy, float l, float w, float r, float g,
                                          float b, float alpha, float s0, float s1, int vb, int ve) {
    float4* d = reinterpret_cast<float4*>(dst);
    d[0] = make_float4(__int_as_float(kind), cx, cy, hx);
    d[1] = make_float4(hy, l, w, r);
    d[2] = make_float4(g, b, alpha, s0);
    d[3] = make_float4(s1, __int_as_float(vb), __int_as_float(ve), 0.0f);
}

__device__ __forceinline__ void store_car(const StriveSceneDraw& J, const Pic& P, float* dst, int row, const float o[4], const Style& st,
                                          float alpha) {
    const float l = unnorm1(J.lw[(long long)(P.a0 + row) * 2 + 0], J.norm.att_mean[0], J.norm.att_std[0]) * P.sl;
    const float w = unnorm1(J.lw[(long long)(P.a0 + row) * 2 + 1], J.norm.att_mean[1], J.norm.att_std[1]) * P.sw;
    store_rec(dst, STRIVE_RENDER_CAR, o[0], o[1], o[2], o[3], l, w, st.r, st.g, st.b, alpha, J.edge_px, J.heading_px, 0, 0);
}

// alpha of the car at window-local step t of T when no trajectories are drawn (:821, :832), in float64, rounded once
__device__ __forceinline__ float fading_alpha(float first, int t, int T) {
    return t == 0 ? first : (float)(0.1 + (1.0 - ((double)t / (double)T)) * 0.2);
}

// resolves picture f; false: a record does not fit the shapes
__device__ bool resolve(const StriveSceneDraw& J, int f, Pic& P, int& flags, int& bidx, int& crop_t, long long& pbase, long long& vbase,
                        int& pcap, int& vcap) {
    const int32_t* pic = J.pictures + (long long)f * PI;
    const int v = pic[0], s_sel = pic[1], t_sel = pic[2];
    pbase = pic[3]; vbase = pic[4]; pcap = pic[5]; vcap = pic[6];
    if (v < 0 || v >= J.NVIEW || pbase < 0 || vbase < 0 || pcap < 0 || vcap < 0 || pbase + pcap > J.NP || vbase + vcap > J.NV) return false;
    const int32_t* V = J.views + (long long)v * VI;
    bidx = V[0]; flags = V[1]; crop_t = V[6];
    if (bidx < 0 || bidx >= J.B) return false;
    const int a0 = J.scene_ptr[bidx], a1 = J.scene_ptr[bidx + 1];
    if (a0 < 0 || a1 < a0 || a1 > J.NA) return false;
    P.a0 = a0; P.n = a1 - a0;
    P.d_src = V[2]; P.d_cnt = V[3]; P.g_src = V[4]; P.g_cnt = V[5];
    if (P.d_src < 0 || P.d_cnt < 0 || P.d_src + P.d_cnt > P.n || P.g_src < 0 || P.g_cnt < 0 || P.g_src + P.g_cnt > P.n) return false;
    const int set = V[7];
    if (set < -1 || set >= STRIVE_SCENE_DRAW_PREDS) return false;
    if (set < 0) {
        P.fut = J.future_gt; P.NS = 1; P.FPT = J.FT;
        P.ft = J.future_stride; P.fs = 0; P.fa = (long long)J.FT * J.future_stride;
    } else {
        if (!J.pred[set] || J.pred_NS[set] < 1 || J.pred_FPT[set] < 0) return false;
        P.fut = J.pred[set]; P.NS = J.pred_NS[set]; P.FPT = J.pred_FPT[set];
        P.ft = 4; P.fs = (long long)P.FPT * 4; P.fa = (long long)P.NS * P.FPT * 4;
    }
    const int NT = J.PT + P.FPT;
    P.gNT = J.PT + J.FT;
    P.traj = (flags & STRIVE_SCENE_DRAW_TRAJ) != 0;
    P.ow = (flags & STRIVE_SCENE_DRAW_OW_GT) != 0;
    if (P.ow && !J.ow_gt) return false;
    if (s_sel >= 0) {                   // a frame of the video: one sample, one step, no ground truth
        if (s_sel >= P.NS || t_sel < 0 || t_sel >= NT) return false;
        P.s0 = s_sel; P.ns = 1; P.t0 = t_sel; P.nt = 1; P.g_cnt = 0;
        P.rb = J.rb_one_off;
    } else {
        P.s0 = 0; P.ns = P.NS; P.t0 = 0; P.nt = NT;
        P.rb = V[8];
    }
    P.rb_gt = J.rb_gt_off;
    if (P.traj && (P.rb < 0 || P.rb + P.nt > J.rb_rows || (P.g_cnt > 0 && (P.rb_gt < 0 || P.rb_gt + P.gNT > J.rb_rows)))) return false;
    P.style = V[9];
    if (P.style < -1 || (P.style >= 0 && (!J.style || P.style + P.d_cnt > J.style_rows))) return false;
    const float* vf = J.view_f + (long long)v * 4;
    P.b0 = vf[0]; P.b1 = vf[1]; P.sl = vf[2]; P.sw = vf[3];
    // the slot holds every candidate: the host sized it from the same shapes
    const long long steps = (long long)P.g_cnt * P.gNT + (long long)P.d_cnt * P.ns * P.nt;
    const long long need_p = P.traj ? steps + P.g_cnt + (long long)P.d_cnt * P.ns + P.d_cnt : steps;
    const long long need_v = P.traj ? steps : 0;
    return need_p <= pcap && need_v <= vcap;
}

__device__ void draw_picture(const StriveSceneDraw& J, int f, Lds& S) {
    const int tid = threadIdx.x;
    Pic P;
    int flags = 0, bidx = 0, crop_t = 0, pcap = 0, vcap = 0;
    long long pbase = 0, vbase = 0;
    const float nan = __int_as_float(0x7fc00000);
    if (!resolve(J, f, P, flags, bidx, crop_t, pbase, vbase, pcap, vcap)) {
        if (tid == 0) {
            for (int c = 0; c < 4; ++c) J.pose[(long long)f * 4 + c] = nan;
            J.mapix[f] = -1;
            J.prim_range[2 * f] = 0; J.prim_range[2 * f + 1] = 0;
            J.status[f] = STRIVE_SCENE_DRAW_BAD_VIEW;
        }
        return;
    }
    int status = 0;
    const long long m = J.map_idx[bidx];
    if (m < 0 || m >= J.M) status |= STRIVE_SCENE_DRAW_BAD_MAP;

    // ---- crop pose ----
    if (flags & STRIVE_SCENE_DRAW_CENTER) {
        const int NTall = J.PT + P.FPT;
        const long long items = (long long)P.n * P.NS * NTall;
        double sx = 0.0, sy = 0.0;
        int cnt = 0;
        for (long long i = tid; i < items; i += SD_THREADS) {
            const int t = (int)(i % NTall);
            const long long r = i / NTall;
            const int s = (int)(r % P.NS), agent = P.a0 + (int)(r / P.NS);
            float in[4];
            load_step(J, agent, t, P.fut, (long long)agent * P.fa + (long long)s * P.fs, P.ft, in);
            if (!is_nan(in[0]) && !is_nan(in[1])) { sx += (double)in[0]; sy += (double)in[1]; ++cnt; }
        }
        S.sx[tid] = sx; S.sy[tid] = sy; S.cnt[tid] = cnt;
        __syncthreads();
        for (int h = SD_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) { S.sx[tid] += S.sx[tid + h]; S.sy[tid] += S.sy[tid + h]; S.cnt[tid] += S.cnt[tid + h]; }
            __syncthreads();
        }
        if (tid == 0) {
            const double c = (double)S.cnt[0];
            S.pose[0] = (float)(S.sx[0] / c); S.pose[1] = (float)(S.sy[0] / c); S.pose[2] = 1.0f; S.pose[3] = 0.0f;
        }
    } else if (tid == 0) {
        const int ct = (flags & STRIVE_SCENE_DRAW_CROP_T) ? crop_t : J.PT - 1;
        if (ct < 0 || ct >= J.PT + J.FT) {
            status |= STRIVE_SCENE_DRAW_BAD_CROP_T;
            for (int c = 0; c < 4; ++c) S.pose[c] = nan;
        } else {
            float in[4];
            load_step(J, P.a0, ct, J.future_gt, (long long)P.a0 * J.FT * J.future_stride, J.future_stride, in);
            for (int c = 0; c < 4; ++c) S.pose[c] = in[c];
        }
    }
    __syncthreads();
    float pose[4];
    for (int c = 0; c < 4; ++c) pose[c] = S.pose[c];

    float* prims = J.prims + pbase * RPF;
    float* verts = J.verts + vbase * 2;
    const long long NG = (long long)P.g_cnt * P.gNT, ND = (long long)P.d_cnt * P.ns * P.nt, N = NG + ND;
    int count = 0, err_agent = 0x7fffffff;

    // ---- one item per step, ground truth first: a disc and a vertex (trajectories) or a car ----
    for (long long base = 0; base < N; base += SD_THREADS) {
        const long long i = base + tid;
        bool valid = false, gt = false;
        int j = 0, t = 0, T = 1;
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i < N) {
            gt = i < NG;
            if (gt) {
                j = (int)(i / P.gNT); t = (int)(i % P.gNT); T = P.gNT;
                valid = gt_step(J, P, pose, j, t, o);
            } else {
                const long long q = i - NG;
                t = (int)(q % P.nt); T = P.nt;
                const long long r = q / P.nt;
                j = (int)(r / P.ns);
                valid = pred_step(J, P, pose, j, (int)(r % P.ns), t, o);
            }
        }
        int total;
        const int pos = count + block_exscan(valid ? 1 : 0, S.wave, total);
        count += total;
        if (valid) {
            const Style st = gt ? gt_style() : style_of(J, P, j);
            if (P.traj) {
                const float* col = J.rainbow + (long long)((gt ? P.rb_gt : P.rb) + t) * 3;
                const float diam = (float)((sqrt((double)st.size) + 1.0) * J.k);
                store_rec(prims + (long long)pos * RPF, STRIVE_RENDER_DISC, o[0], o[1], 0.0f, 0.0f, diam, 0.0f, col[0], col[1], col[2],
                          st.alpha, 0.0f, 0.0f, 0, 0);
                verts[2 * (long long)pos] = o[0];
                verts[2 * (long long)pos + 1] = o[1];
            } else {
                store_car(J, P, prims + (long long)pos * RPF, j, o, st, fading_alpha(st.alpha, t, T));
            }
        }
    }

    if (P.traj) {
        // ---- one item per trajectory: its line over the vertices its steps left ----
        const long long R = (long long)P.g_cnt + (long long)P.d_cnt * P.ns;
        long long vstart = 0;
        for (long long base = 0; base < R; base += SD_THREADS) {
            const long long r = base + tid;
            int nv = 0, j = 0;
            bool gt = false;
            if (r < R) {
                float o[4];
                gt = r < P.g_cnt;
                if (gt) {
                    j = (int)r;
                    for (int t = 0; t < P.gNT; ++t) nv += gt_step(J, P, pose, j, t, o) ? 1 : 0;
                } else {
                    const long long q = r - P.g_cnt;
                    j = (int)(q / P.ns);
                    for (int t = 0; t < P.nt; ++t) nv += pred_step(J, P, pose, j, (int)(q % P.ns), t, o) ? 1 : 0;
                }
            }
            int tot_v, tot_l;
            const long long v0 = vstart + block_exscan(nv, S.wave, tot_v);
            const int pos = count + block_exscan(nv > 0 ? 1 : 0, S.wave, tot_l);
            vstart += tot_v;
            count += tot_l;
            if (nv > 0) {
                const Style st = gt ? gt_style() : style_of(J, P, j);
                store_rec(prims + (long long)pos * RPF, STRIVE_RENDER_POLYLINE, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, st.r, st.g, st.b, st.alpha,
                          (float)((double)st.width * J.k), 0.0f, (int)(vbase + v0), (int)(vbase + v0 + nv));
            }
        }
        // ---- one item per drawn agent: the car at its first observed step of the window's first sample ----
        for (int base = 0; base < P.d_cnt; base += SD_THREADS) {
            const int j = base + tid;
            bool found = false;
            float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (j < P.d_cnt) {
                for (int t = 0; t < P.nt && !found; ++t) {
                    pred_step(J, P, pose, j, 0, t, o);
                    found = !is_nan(o[0]);
                }
                if (!found && j < err_agent) err_agent = j;
            }
            int total;
            const int pos = count + block_exscan(found ? 1 : 0, S.wave, total);
            count += total;
            if (found) {
                const Style st = style_of(J, P, j);
                store_car(J, P, prims + (long long)pos * RPF, j, o, st, st.alpha);
            }
        }
        __syncthreads();
        S.cnt[tid] = err_agent;
        __syncthreads();
        for (int h = SD_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) S.cnt[tid] = S.cnt[tid + h] < S.cnt[tid] ? S.cnt[tid + h] : S.cnt[tid];
            __syncthreads();
        }
        err_agent = S.cnt[0];
    }

    if (tid == 0) {
        // (without a crop pose nothing has a crop value: that is BAD_CROP_T's doing, not the agents')
        if (err_agent != 0x7fffffff && !(status & STRIVE_SCENE_DRAW_BAD_CROP_T)) status |= STRIVE_SCENE_DRAW_NO_STEP | ((err_agent + 1) << 8);
        for (int c = 0; c < 4; ++c) J.pose[(long long)f * 4 + c] = pose[c];
        J.mapix[f] = (m < 0 || m >= J.M) ? -1 : (int)m;
        J.prim_range[2 * f] = (int)pbase;
        J.prim_range[2 * f + 1] = (int)pbase + count;
        J.status[f] = status;
    }
}

__global__ __launch_bounds__(SD_THREADS) void scene_draw_kernel(StriveSceneDraw J) {
    __shared__ Lds S;
    for (int f = blockIdx.x; f < J.F; f += gridDim.x) {
        draw_picture(J, f, S);
        __syncthreads();
    }
}
}  // namespace

extern "C" int strive_scene_draw_tables(const StriveSceneDraw* job, strive_stream_t stream) {
    STRIVE_CHECK_ARG(job, "null argument");
    STRIVE_CHECK_ARG(job->F >= 0 && job->NVIEW >= 0 && job->NP >= 0 && job->NV >= 0 && job->NA >= 0 && job->B >= 0 && job->M >= 0, "bad sizes");
    STRIVE_CHECK_ARG(job->PT >= 1 && job->FT >= 0 && job->past_stride >= 4 && job->future_stride >= 4, "bad trajectory shapes");
    if (job->F == 0) return 0;
    STRIVE_CHECK_ARG(job->past_gt && job->lw && (job->FT == 0 || job->future_gt) && job->scene_ptr && job->map_idx, "missing batch tensors");
    STRIVE_CHECK_ARG(job->views && job->view_f && job->pictures && job->rainbow, "missing view tables");
    STRIVE_CHECK_ARG(job->pose && job->mapix && job->prim_range && job->status && (job->NP == 0 || job->prims) && (job->NV == 0 || job->verts),
                     "missing output tables");
    STRIVE_CHECK_ARG((((uintptr_t)job->prims) & 15) == 0, "the primitive table must be 16-byte aligned");
    STRIVE_CHECK_ARG(job->rb_rows >= 1 && job->rb_one_off >= 0 && job->rb_one_off < job->rb_rows, "the marker colour table lacks the frame row");
    const int grid = job->F < 4096 ? job->F : 4096;
    hipLaunchKernelGGL(scene_draw_kernel, dim3(grid), dim3(SD_THREADS), 0, (hipStream_t)stream, *job);
    STRIVE_CHECK_LAUNCH();
    return 0;
}
