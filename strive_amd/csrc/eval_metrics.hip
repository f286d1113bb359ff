// Evaluation metrics: the rotated-box IoU, the three batched evaluation kernels (planner, adversarial scenarios, traffic model)
// the verdict and screening kernels of the drivers, and the k-means step of the scenario clustering.  float64 code that no
// optimisation loop calls; the formulas and the steps the kernels share live in eval_dev.h and are named here where they are used:
// scene_span (a scene's agents and status 2 / 3), sample_grid on grid_ratios (the sampling grid of check_on_layer), road_samples /
// wave_off_road / off_road (the drivable test of a frame), wave_pair_vote (one agent against the agents after it), valid_frames /
// add_valid_rows (the rows a grid is formed from), unnorm_pose / unnorm_lw on EvalNorm (normalised inputs).
#include "eval_dev.h"

// =============================================================================================
// Rotated-rectangle IoU of vehicle boxes (the success / collision-metric tests of the optimisation loops:
// reference src/losses/adv_gen_nusc.py:517-623 builds shapely polygons from get_corners
// (src/datasets/nuscenes_utils.py:416-428) and evaluates intersection.area / union.area per (agent, step) in Python).
// One thread per box pair, float64: corners = R(atan2(hy, hx)) * (+-l/2, +-w/2) + (x, y); the first quadrilateral is
// clipped against the four edges of the second (Sutherland-Hodgman, <= 8 vertices) and the areas come from the
// shoelace formula.  A pair with a NaN in either pose yields NaN (the reference skips such frames).
// =============================================================================================
__global__ __launch_bounds__(256) void rect_iou_kernel(const float* __restrict__ box_a, const float* __restrict__ lw_a,
                                                         const float* __restrict__ box_b, const float* __restrict__ lw_b, int P,
                                                         double* __restrict__ iou) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const float* a = box_a + (size_t)p * 4;
    const float* b = box_b + (size_t)p * 4;
    iou[p] = (nan4(a) || nan4(b)) ? eval_nan() : box_iou(a, lw_a + (size_t)p * 2, b, lw_b + (size_t)p * 2);
}

extern "C" int strive_rect_iou(const float* box_a, const float* lw_a, const float* box_b, const float* lw_b, int32_t P,
                               double* iou, strive_stream_t stream) {
    STRIVE_CHECK_ARG(box_a && lw_a && box_b && lw_b && iou, "null argument");
    if (P <= 0) return 0;
    hipLaunchKernelGGL(rect_iou_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, box_a, lw_a, box_b, lw_b, P, iou);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// =============================================================================================
// Planner evaluation metrics (reference src/eval_planner.py:114-218, compute_metrics) for B scenes in one launch, float64.
// One workgroup per scene.  The (agent, fine step) pairs are strided over the threads: each up-samples the ego's plan and
// the agent's future at its fine step (interp_traj, :625-644: half-pixel linear taps, heading renormalised; the plan in
// float64, the other agents in fp32 as the reference holds them, so a NaN neighbour gives a NaN fine frame), forms the
// two boxes and their IoU, and a hit (IoU > 0.02, NaN frames skipped) enters the integer key fine_step * n + agent into a
// shared minimum.  The smallest key IS (coll_time, coll_agt) of check_single_veh_coll + np.amin / np.argmin: the earliest
// first hit, and among the agents hitting then the lowest index; an integer minimum does not depend on the order of
// evaluation.  Thread 0 then walks the coarse frames 0 upwards (collision index, relative speed at impact, the three
// acceleration series), so a scene's outputs do not depend on what else is in the batch.
//   out_i (B,5): did_collide, coll_time (T*scale without a hit), coll_agt, coll_idx, number of acceleration frames
//   out_d (B,7): coll_vel (NaN without a hit), then sum and max of |accel|, of the forward and of the lateral acceleration
//   status (B) : 0; 1 for a scene without other agents, 2 for offsets outside ``others`` (nothing else is written for either)
// =============================================================================================
__global__ __launch_bounds__(256) void planner_eval_kernel(const double* __restrict__ plan, const float* __restrict__ others,
                                                             const int32_t* __restrict__ ptr, const float* __restrict__ lw_ego,
                                                             const float* __restrict__ lw_others, int NR, int T, int scale, double dt,
                                                             int32_t* __restrict__ out_i, double* __restrict__ out_d,
                                                             int32_t* __restrict__ status) {
    __shared__ int s_key;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int TO = T * scale;
    int a0, n;
    if (scene_span(ptr, b, NR, a0, n) != 0) {
        if (tid == 0) status[b] = n == 0 ? 1 : 2;        // 2: ptr does not lie inside ``others`` (nothing is read)
        return;
    }
    if (tid == 0) {
        s_key = EVAL_NO_KEY;
        status[b] = 0;
    }
    __syncthreads();
    const double* pl = plan + (size_t)b * T * 4;
    const float rs_f = (float)(1.0 / (double)scale);
    const double rs_d = 1.0 / (double)scale;
    int best = EVAL_NO_KEY;
    for (int e = tid; e < n * TO; e += 256) {
        const int j = e / n, al = e - j * n;            // e IS the key fine_step * n + agent
        float u[4];
        double g[4];
        fine_frame(others + (size_t)(a0 + al) * T * 4, T, j, rs_f, u);       // the other agent in fp32, the ego's plan in float64
        if (nan4(u)) continue;
        fine_frame(pl, T, j, rs_d, g);
        if (boxes_hit(g, lw_ego + (size_t)b * 2, u, lw_others + (size_t)(a0 + al) * 2)) {
            best = e;                                   // this thread's keys only grow from here
            break;
        }
    }
    if (best != EVAL_NO_KEY) atomicMin(&s_key, best);
    __syncthreads();
    if (tid != 0) return;
    const int key = s_key;
    const bool did = key != EVAL_NO_KEY;
    const int coll_time = did ? key / n : TO;
    const int coll_agt = did ? key - coll_time * n : 0;
    int coll_idx = did ? coarse_index(coll_time, dt, scale) : T - 1;
    coll_idx = coll_idx > T - 1 ? T - 1 : coll_idx;
    int32_t* oi = out_i + (size_t)b * 5;
    double* od = out_d + (size_t)b * 7;
    const double coll_vel = did ? rel_speed(pl, others + (size_t)(a0 + coll_agt) * T * 4, coll_idx, dt) : eval_nan();
    // comfort over the pre-crash frames 0..coll_idx (:176-216)
    int cnt = 0;
    double sum[3] = {0.0, 0.0, 0.0}, mx[3] = {0.0, 0.0, 0.0};
    if (coll_idx > 1) accel_series(pl, coll_idx + 1, dt, sum, mx, cnt);
    oi[0] = did ? 1 : 0;
    oi[1] = coll_time;
    oi[2] = coll_agt;
    oi[3] = coll_idx;
    oi[4] = cnt;
    od[0] = coll_vel;
    for (int c = 0; c < 3; ++c) {
        od[1 + 2 * c] = sum[c];
        od[2 + 2 * c] = mx[c];
    }
}

extern "C" int strive_planner_eval_metrics(const double* plan, const float* others, const int32_t* ptr, const float* lw_ego,
                                           const float* lw_others, int32_t B, int32_t NR, int32_t T, int32_t scale, double dt,
                                           int32_t* out_i, double* out_d, int32_t* status, strive_stream_t stream) {
    STRIVE_CHECK_ARG(plan && others && ptr && lw_ego && lw_others && out_i && out_d && status, "null argument");
    STRIVE_CHECK_ARG(T >= 2, "T must be at least 2");
    STRIVE_CHECK_ARG(scale >= 1, "bad scale");
    STRIVE_CHECK_ARG(dt > 0.0, "bad dt");
    // (the key fine_step * n + agent and the strided loop counter, which runs up to 255 past the last key, are ints)
    STRIVE_CHECK_ARG(NR >= 0 && (int64_t)(NR > 0 ? NR : 1) * T * scale < 0x7fffffffll - 256,
                     "NR * T * scale does not fit the collision key");
    if (B <= 0) return 0;
    hipLaunchKernelGGL(planner_eval_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, plan, others, ptr, lw_ego, lw_others, NR, T,
                       scale, dt, out_i, out_d, status);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// =============================================================================================
// Adversarial-scenario evaluation (reference src/eval_adv_gen.py:339-513 compute_metrics and :116-168 compute_coll_feat) for
// B scenes in ONE launch, float64 on the fp32 inputs, one workgroup per scene; nothing is shared between scenes, every
// cross-thread result is an integer minimum / flag or is added by one thread in index order, so a scene's outputs are
// bit-identical whatever else is in the batch.  Per scene, in the reference's order:
//   1. ego (agent 0) against every other agent at the coarse steps (check_single_veh_coll, src/losses/adv_gen_nusc.py:517-565:
//      hit = IoU > 0.02, frames holding NaN skipped): the key step * (n-1) + agent enters a shared integer minimum, which IS
//      (np.amin, np.argmin) of the first-hit times: CT (T without a hit) and coll_agt = argmin + 1.  The effective attacker
//      is coll_agt after a hit, else the JSON's attack_agt; the "others" are every agent but the ego and that attacker.
//   2. CT > 0: check_pairwise_veh_coll (:567-623) on the non-ego agents over steps [0, CT).  The reference leaves the j loop
//      once agent i is marked and the t loop at the first hit, so its coll_count is incremented exactly once per marked agent:
//      coll_count == number of agents i that overlap SOME j > i at SOME step.  That set does not depend on the order of
//      evaluation: the workgroup strides over all (pair, step) and sets flags.  (A NaN pose gives a NaN IoU, which is no hit.)
//   3. CT > 0 and a map: compute_coll_rate_env_from_traj (src/losses/traffic_model.py:421-463) -> check_on_layer
//      (src/datasets/nuscenes_utils.py:266-298) on the frames [0, CT) of ALL agents that hold no NaN.  The sampling grid is
//      L = round(mean_l / mean(dx)), W likewise, the mean of lw over the valid (agent, step) rows of the scene (the reference's
//      expanded tensor), formed here in float64 from the per-agent frame counts; samples are (linspace(-1,1,L) * l) / 2 in
//      fp32 from the caller's table, pixels by crop_dev.h (fp64 divide, round half even, out of bounds -> pixel (0,0)); a
//      frame is off road when fp32(count) / fp32(L*W) < fp32(1 - 0.05).  (sample_grid; one thread per frame walks road_samples
//      and asks off_road.)
//   4. compute_accels (:323-337) over [0, CT): the attacker when CT > 2; the others' series concatenated in agent order.
//   5. log_normal (src/losses/common.py:26-42) of the attacker's latent row and of the others' rows.
//   6. planner fit over [0, CT): position error, angle between the unit headings (dot product clamped to [-1, 1]).
//   7. want_feat: compute_coll_feat -- ego and others up-sampled x5 in fp32 (interp_traj, headings renormalised), first hit
//      per agent at the fine steps as in 1., the attacker's pose in the ego's frame at that fine step (transform2frame,
//      src/utils/transforms.py:78-139), rel_s from the coarse frames at lr_coll_t = int((t_fine * (dt / 5)) / dt).
//   out_i (B, 20): adv_collide, coll_t, coll_agt, atk_agt (effective), num_coll_veh, num_traj_veh, env_coll_atk, env_coll_others,
//                  n_others, env_L, env_W, atk_accel_cnt, other_accel_cnt, ll_other_cnt, fit_cnt, feat_status (-1 not asked,
//                  0 found, 1 no fine-step contact), fine_t, fine_agt (row among the others), lr_coll_t, env_frames; -1 = absent
//   out_d (B, 26): attacker (sum, max) of |accel|, forward, lateral; the same six for the others; ll_atk, ll_other_sum,
//                  fit_pos_sum, fit_ang_rad_sum, fit_ang_deg_sum, hvec (2), angvec (2), h, ang, rel_s, env_mean_l, env_mean_w;
//                  NaN = absent
//   status (B)   : 0 written; 1 ego only; 2 offsets / attack_agt / map index out of range; 3 more than 63 others; 4 the
//                  sampling grid exceeds the caller's linspace table (outputs untouched for every non-zero status)
// =============================================================================================
#define SE_NI 20
#define SE_ND 26
#define SE_MAX_OTHERS 63
#define SE_MAX_PAIRS (SE_MAX_OTHERS * (SE_MAX_OTHERS - 1) / 2)
#define SE_FEAT_SCALE 5
#define SE_LOG_SQRT_2PI 0.91893853320467274178      // math.log(math.sqrt(2 * math.pi))

struct ScenarioEvalArgs {
    const float* fut; const int32_t* ptr; const float* lw; const int32_t* atk_agt; const double* dt;
    const float* z; const float* mu; const float* var; int D;
    const float* plan_fit; const int32_t* has_fit;
    int has_map; const int32_t* mapix; const float* lin_tab; int lin_max;
    const int32_t* want_feat;
    int NA, T;
    int32_t* out_i; double* out_d; int32_t* status;
};

__global__ __launch_bounds__(256) void scenario_eval_kernel(ScenarioEvalArgs A, StriveMap map) {
#pragma clang fp contract(off)
    __shared__ int s_key, s_fkey, s_L, s_W, s_env_ok;
    __shared__ int s_mark[SE_MAX_OTHERS + 1], s_env[SE_MAX_OTHERS + 1], s_cnt[SE_MAX_OTHERS + 1], s_acnt[SE_MAX_OTHERS + 1];
    __shared__ double s_ll[SE_MAX_OTHERS + 1], s_asum[SE_MAX_OTHERS + 1][3], s_amax[SE_MAX_OTHERS + 1][3];
    __shared__ unsigned char s_pi[SE_MAX_PAIRS], s_pj[SE_MAX_PAIRS];
    const double kNaN = eval_nan();
    const int b = blockIdx.x, tid = threadIdx.x, T = A.T;
    int a0, n;
    int st = scene_span(A.ptr, b, A.NA, a0, n);               // (the map index comes last: a scene of the ego alone has status 1)
    const int nO = n - 1;
    if (st == 0) {
        if (n == 1) st = 1;
        else if (nO > SE_MAX_OTHERS) st = 3;
        else if (A.atk_agt[b] < 0 || A.atk_agt[b] >= n) st = 2;
        else if (A.has_map && !map_index_ok(A.mapix[b], map.M)) st = 2;
    }
    if (st != 0) {
        if (tid == 0) A.status[b] = st;
        return;
    }
    const float* fut = A.fut + (size_t)a0 * T * 4;         // (n, T, 4), the ego first
    const float* lw = A.lw + (size_t)a0 * 2;
    const double dt = A.dt[b];
    if (tid == 0) {
        s_key = EVAL_NO_KEY;
        s_fkey = EVAL_NO_KEY;
        s_env_ok = 1;
    }
    if (tid <= SE_MAX_OTHERS) {
        s_mark[tid] = 0;
        s_env[tid] = 0;
    }
    __syncthreads();

    // ---- 1. ego against the others, coarse steps ----
    for (int e = tid; e < nO * T; e += 256) {
        const int t = e / nO, al = e - t * nO;               // e IS the key step * nO + agent
        const float* pe = fut + (size_t)t * 4;
        const float* po = fut + ((size_t)(al + 1) * T + t) * 4;
        if (boxes_hit(pe, lw, po, lw + (al + 1) * 2)) {
            atomicMin(&s_key, e);                            // this thread's keys only grow from here
            break;
        }
    }
    __syncthreads();
    const int key = s_key;
    const bool did = key != EVAL_NO_KEY;
    const int CT = did ? key / nO : T;
    const int coll_agt = did ? key - CT * nO + 1 : 1;        // np.argmin of an all-T array is 0
    const int atk = did ? coll_agt : A.atk_agt[b];
    const int n_others = nO - (atk != 0 ? 1 : 0);

    // ---- 2. pairs of non-ego agents before the crash ----
    const int npairs = nO * (nO - 1) / 2;
    if (CT > 0 && npairs > 0) {
        if (tid < nO) {
            int off = tid * (2 * nO - tid - 1) / 2;
            for (int j = tid + 1; j < nO; ++j, ++off) {
                s_pi[off] = (unsigned char)tid;
                s_pj[off] = (unsigned char)j;
            }
        }
        __syncthreads();
        for (int e = tid; e < npairs * CT; e += 256) {
            const int p = e / CT, t = e - p * CT;
            const int i = s_pi[p], j = s_pj[p];
            const float* pa = fut + ((size_t)(i + 1) * T + t) * 4;
            const float* pb = fut + ((size_t)(j + 1) * T + t) * 4;
            if (boxes_hit(pa, lw + (i + 1) * 2, pb, lw + (j + 1) * 2)) atomicOr(&s_mark[i], 1);
        }
    }

    // ---- 3. drivable fraction of every valid frame before the crash ----
    const bool do_env = CT > 0 && A.has_map;
    if (do_env) {
        if (tid < n) {
            int c = 0;
            for (int t = 0; t < CT; ++t) c += nan4(fut + ((size_t)tid * T + t) * 4) ? 0 : 1;
            s_cnt[tid] = c;
        }
        __syncthreads();
        if (tid == 0) {
            long long tot = 0;
            double sl = 0.0, sw = 0.0;
            for (int a = 0; a < n; ++a) {
                tot += s_cnt[a];
                sl += (double)s_cnt[a] * (double)lw[a * 2 + 0];
                sw += (double)s_cnt[a] * (double)lw[a * 2 + 1];
            }
            int L, W;
            double mean[2] = {kNaN, kNaN}, ratio[2];
            if (!sample_grid(tot, sl, sw, map, A.lin_max, mean, ratio, L, W)) s_env_ok = 0;
            s_L = L;
            s_W = W;
            s_ll[0] = mean[0];                                    // (scratch: s_ll is filled in step 5)
            s_ll[1] = mean[1];
        }
        __syncthreads();
        if (!s_env_ok) {
            if (tid == 0) A.status[b] = 4;
            return;
        }
    }
    double env_ml = kNaN, env_mw = kNaN;
    int env_frames = -1;
    if (do_env) {
        const int L = s_L, W = s_W;
        env_ml = s_ll[0];
        env_mw = s_ll[1];
        const int m = A.mapix[b];
        for (int e = tid; L > 0 && e < n * CT; e += 256) {          // (one thread per frame: road_samples without a wave)
            const int a = e / CT, t = e - a * CT;
            const float* p = fut + ((size_t)a * T + t) * 4;
            if (nan4(p)) continue;
            if (off_road(road_samples(map, m, p, lw + a * 2, A.lin_tab, L, W, 0, 1), L * W)) atomicOr(&s_env[a], 1);
        }
        if (tid == 0) {
            env_frames = 0;
            for (int a = 0; a < n; ++a) env_frames += s_cnt[a];
        }
    }
    __syncthreads();                                          // s_ll scratch read, s_mark / s_env complete

    // ---- 4. accelerations and 5. latent log-likelihood, one agent per thread ----
    if (tid < n) {
        double sum[3] = {0.0, 0.0, 0.0}, mx[3] = {0.0, 0.0, 0.0};
        int cnt = 0;
        if (CT > 2) accel_series(fut + (size_t)tid * T * 4, CT, dt, sum, mx, cnt);
        s_acnt[tid] = cnt;
        for (int c = 0; c < 3; ++c) {
            s_asum[tid][c] = sum[c];
            s_amax[tid][c] = mx[c];
        }
        double ll = kNaN;
        if (A.z) {
            ll = 0.0;
            const size_t r = (size_t)(a0 + tid) * A.D;
            for (int d = 0; d < A.D; ++d) {
                const double x = (double)A.z[r + d], m = (double)A.mu[r + d], v = (double)A.var[r + d];
                ll += -log(sqrt(v)) - SE_LOG_SQRT_2PI - ((x - m) * (x - m)) / (2.0 * v);
            }
        }
        s_ll[tid] = ll;
    }

    // ---- 7. (first part) fine-step contact ----
    const bool feat = A.want_feat[b] != 0;
    const int TO = T * SE_FEAT_SCALE;
    const float rs_f = (float)(1.0 / (double)SE_FEAT_SCALE);
    if (feat) {
        for (int e = tid; e < nO * TO; e += 256) {
            const int j = e / nO, al = e - j * nO;
            float g[4], u[4];
            fine_frame(fut + (size_t)(al + 1) * T * 4, T, j, rs_f, u);
            if (nan4(u)) continue;
            fine_frame(fut, T, j, rs_f, g);
            if (boxes_hit(g, lw, u, lw + (al + 1) * 2)) {
                atomicMin(&s_fkey, e);
                break;
            }
        }
    }
    __syncthreads();
    if (tid != 0) return;

    int32_t* oi = A.out_i + (size_t)b * SE_NI;
    double* od = A.out_d + (size_t)b * SE_ND;
    for (int c = 0; c < SE_NI; ++c) oi[c] = -1;
    for (int c = 0; c < SE_ND; ++c) od[c] = kNaN;
    oi[0] = did ? 1 : 0;
    oi[1] = CT;
    oi[2] = coll_agt;
    oi[3] = atk;
    oi[8] = n_others;
    if (CT > 0) {
        int marked = 0;
        for (int i = 0; i < nO; ++i) marked += s_mark[i];
        oi[4] = marked;
        oi[5] = nO;
    }
    if (do_env) {
        int oth = 0;
        for (int a = 1; a < n; ++a) oth += (a != atk) ? s_env[a] : 0;
        oi[6] = s_env[atk];
        oi[7] = oth;
        oi[9] = s_L;
        oi[10] = s_W;
        oi[19] = env_frames;
        od[24] = env_ml;
        od[25] = env_mw;
    }
    // accelerations: the attacker's block, then the others' series in agent order
    oi[11] = s_acnt[atk];
    if (s_acnt[atk] > 0)
        for (int c = 0; c < 3; ++c) {
            od[2 * c] = s_asum[atk][c];
            od[2 * c + 1] = s_amax[atk][c];
        }
    {
        int cnt = 0;
        double sum[3] = {0.0, 0.0, 0.0}, mx[3] = {0.0, 0.0, 0.0};
        for (int a = 1; a < n; ++a) {
            if (a == atk || s_acnt[a] == 0) continue;
            for (int c = 0; c < 3; ++c) {
                sum[c] += s_asum[a][c];
                const double v = s_amax[a][c];
                mx[c] = (cnt == 0 || v > mx[c] || v != v) ? v : mx[c];
            }
            cnt += s_acnt[a];
        }
        oi[12] = cnt;
        if (cnt > 0)
            for (int c = 0; c < 3; ++c) {
                od[6 + 2 * c] = sum[c];
                od[7 + 2 * c] = mx[c];
            }
    }
    if (A.z) {
        od[12] = s_ll[atk];
        double sum = 0.0;
        for (int a = 1; a < n; ++a) sum += (a != atk) ? s_ll[a] : 0.0;
        oi[13] = n_others;
        if (n_others > 0) od[13] = sum;
    }
    if (A.has_fit[b]) {
        const float* pf = A.plan_fit + (size_t)b * T * 4;
        double sp = 0.0, sr = 0.0, sd = 0.0;
        for (int t = 0; t < CT; ++t) {
            double pos, ang;
            pose_err(fut + t * 4, pf + t * 4, pos, ang);
            sp += pos;
            sr += ang;
            sd += ang * EVAL_DEG_PER_RAD;
        }
        oi[14] = CT;
        od[14] = sp;
        od[15] = sr;
        od[16] = sd;
    }
    if (feat) {
        const int fkey = s_fkey;
        if (fkey == EVAL_NO_KEY) {
            oi[15] = 1;
        } else {
            const int ft = fkey / nO, fa = fkey - ft * nO;
            float g[4], u[4];
            fine_frame(fut, T, ft, rs_f, g);
            fine_frame(fut + (size_t)(fa + 1) * T * 4, T, ft, rs_f, u);
            // transform2frame(ego, attacker): heading Rp Rf, position Rf (p - f)
            const double fc = (double)g[2], fs = (double)g[3], pc = (double)u[2], ps = (double)u[3];
            const double hc = pc * fc + ps * fs, hs = ps * fc - pc * fs;
            const double ddx = (double)u[0] - (double)g[0], ddy = (double)u[1] - (double)g[1];
            const double lx = fc * ddx + fs * ddy, ly = -fs * ddx + fc * ddy;
            const double ln = sqrt(lx * lx + ly * ly);
            const int lr = coarse_index(ft, dt, SE_FEAT_SCALE);
            oi[15] = 0;
            oi[16] = ft;
            oi[17] = fa;
            oi[18] = lr;
            od[17] = hc;
            od[18] = hs;
            od[19] = lx / ln;
            od[20] = ly / ln;
            od[21] = atan2(hs, hc);
            od[22] = atan2(ly / ln, lx / ln);
            od[23] = rel_speed(fut, fut + (size_t)(fa + 1) * T * 4, lr, dt);
        }
    }
    A.status[b] = 0;
}

extern "C" int strive_scenario_eval_metrics(const float* fut, const int32_t* ptr, const float* lw, const int32_t* atk_agt,
                                            const double* dt, const float* z, const float* mu, const float* var, int32_t D,
                                            const float* plan_fit, const int32_t* has_fit, const StriveMap* map,
                                            const int32_t* mapix, const float* lin_tab, int32_t lin_max, const int32_t* want_feat,
                                            int32_t B, int32_t NA, int32_t T, int32_t* out_i, double* out_d, int32_t* status,
                                            strive_stream_t stream) {
    STRIVE_CHECK_ARG(fut && ptr && lw && atk_agt && dt && plan_fit && has_fit && want_feat && out_i && out_d && status, "null argument");
    STRIVE_CHECK_ARG((z && mu && var) || (!z && !mu && !var), "z, mu and var must be given together");
    STRIVE_CHECK_ARG(!z || (D >= 1 && D <= 64), "latent size must be 1..64");
    STRIVE_CHECK_ARG(!map || (mapix && lin_tab && lin_max >= 1), "a map needs mapix and the linspace table");
    STRIVE_CHECK_ARG(!map || eval_map_ok(map), "bad map");
    STRIVE_CHECK_ARG(T >= 2 && T <= 4096, "T must be 2..4096");
    STRIVE_CHECK_ARG(NA >= 0, "bad NA");
    if (B <= 0) return 0;
    ScenarioEvalArgs A;
    A.fut = fut; A.ptr = ptr; A.lw = lw; A.atk_agt = atk_agt; A.dt = dt;
    A.z = z; A.mu = mu; A.var = var; A.D = D;
    A.plan_fit = plan_fit; A.has_fit = has_fit;
    A.has_map = map ? 1 : 0; A.mapix = mapix; A.lin_tab = lin_tab; A.lin_max = lin_max;
    A.want_feat = want_feat;
    A.NA = NA; A.T = T;
    A.out_i = out_i; A.out_d = out_d; A.status = status;
    StriveMap m;
    memset(&m, 0, sizeof(m));
    if (map) m = *map;
    hipLaunchKernelGGL(scenario_eval_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, A, m);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// =============================================================================================
// Traffic-model evaluation (reference src/test_traffic.py:84-277 and the metric functions it calls in
// src/losses/traffic_model.py) for ONE prediction set pred (NA,NS,T,4) of B scenes in one host call without a host
// synchronisation: float64 on the fp32 inputs, one workgroup per scene (up to 8 with many samples, each owning whole items).  Poses, ground truth and vehicle sizes arrive
// NORMALISED and are unnormalised in fp32 exactly as MeanStdNormalizer.unnormalize does (v * std + mean, src/datasets/utils.py:
// 75-90), so pixel selection and box corners start from the fp32 values the reference sees.  Four optional groups (`groups`
// bits 1, 2, 4, 8); a group that is not asked for leaves its outputs untouched:
//   err  (compute_err, :120-164, sample 0, T == Tg): pos_err / ang_err (NA,Tg), NaN where vis != 1; unit headings, the dot
//        product clamped to [-1, 1] before acos, degrees.
//   disp (compute_disp_err, :297-364): per scene for its ego ptr[b] over Tc = min(T, Tg): pos_minADE, pos_minFDE, ang_minADE,
//        ang_minFDE (a NaN sample makes the minimum NaN, as torch.min does) and APD = 2 sum_{s<s'} sum_t |p_s - p_s'| /
//        (NS (NS-1) Tc), 0/0 = NaN for NS = 1.  One thread walks a sample's steps in order; the (s, s', t) terms are strided over
//        the workgroup and the 256 partial sums added by one thread in thread order: no NS x NS x T array anywhere.
//   veh  (compute_coll_rate_veh, :465-545): did_collide_veh (NA,NS): agent i overlaps (IoU > 0.02) some agent j > i of the same
//        scene at some step of sample s; a frame with a NaN in either pose is no hit.  The reference's early exits make
//        coll_count the number of set flags and the set does not depend on the order of evaluation: ONE WAVE owns a flag, its
//        lanes stride over (j, t) and vote (wave_pair_vote, here without the centre-distance reject), lane 0 writes -- no atomics.
//   env  (compute_coll_rate_env, :366-419 -> check_on_layer, src/datasets/nuscenes_utils.py:266-298): did_collide_map (B,NS)
//        with env_ego_only, else (NA,NS): some valid frame has fp32(count) / fp32(L W) < fp32(0.95) on raster layer 0.  One
//        wave owns a flag, walks the frames in order, its lanes stride over the L x W samples (crop_dev.h: fp32 grid, float64
//        divide, round half even, outside -> pixel (0,0)) and add their integer counts (wave_off_road).  The grid couples the batch: L =
//        round(mean_l / mean(dx)), W likewise, mean over the valid (agent, sample, step) rows of the whole call (ego rows only
//        with env_ego_only), mean(dx) over all entries of the map's dx.  traffic_eval_grid_kernel (one workgroup, launched
//        first) forms it in float64: a thread adds count * size for the agents tid, tid + 256, ... in that order (add_valid_rows),
//        one thread adds the 256 partial sums in thread order (te_row_sums); on grid_ratios it rounds with a rule of its own, which
//        saturates and reports where sample_grid refuses.  grid_i = (L, W, valid rows clamped to int32), grid_d = the two ratios before
//        rounding (NaN without a valid row: then there is no grid and no collision).  With bit 16 of `groups` the caller's grid_i
//        is used as given and the first launch is skipped.
//   status (B): 0 written; 2 agent offsets leave the arrays or n < 1; 3 map index out of range; 4 the grid is outside
//        1..lin_max along an axis (every scene of the call).  Outputs are untouched for a scene with a non-zero status; rows of
//        such a scene still enter the grid means when they can be addressed (with env_ego_only: when its offsets are valid).
// Given the grid, a scene's outputs are bit-identical whatever else is in the batch.
// =============================================================================================
#define TE_ERR 1
#define TE_DISP 2
#define TE_VEH 4
#define TE_ENV 8
#define TE_GRID_GIVEN 16
#define TE_NT 256

struct TrafficEvalArgs {
    const float* pred; const float* gt; const float* vis; const int32_t* ptr; const float* lw;
    EvalNorm nrm;
    const int32_t* mapix; const float* lin_tab; int lin_max;
    int groups, ego_only;
    int B, NA, NS, T, Tg;
    double* pos_err; double* ang_err; double* disp; int32_t* did_veh; int32_t* did_map;
    int32_t* grid_i; double* grid_d; int32_t* status;
};

// The valid-row count and the two size sums of a sampling grid from the TE_NT per-thread partials: thread 0 adds them in thread
// order (the totals are valid in thread 0 only; holds a barrier, so the whole workgroup calls it).
__device__ __forceinline__ void te_row_sums(int tid, long long cnt, double sl, double sw, long long* s_cnt, double* s_l, double* s_w,
                                            long long& tot, double& tl, double& tw) {
#pragma clang fp contract(off)
    s_cnt[tid] = cnt;
    s_l[tid] = sl;
    s_w[tid] = sw;
    __syncthreads();
    tot = 0;
    tl = 0.0;
    tw = 0.0;
    if (tid != 0) return;
    for (int i = 0; i < TE_NT; ++i) {
        tot += s_cnt[i];
        tl += s_l[i];
        tw += s_w[i];
    }
}

// torch.min over values that may hold NaN: NaN wins
__device__ __forceinline__ double te_min(double m, double v) { return (m != m || v != v) ? (m + v) : (v < m ? v : m); }

__global__ __launch_bounds__(TE_NT) void traffic_eval_grid_kernel(TrafficEvalArgs A, StriveMap map) {
#pragma clang fp contract(off)
    __shared__ long long s_cnt[TE_NT];
    __shared__ double s_l[TE_NT], s_w[TE_NT];
    const int tid = threadIdx.x;
    const int items = A.ego_only ? A.B : A.NA;
    const size_t frames = (size_t)A.NS * A.T;
    long long cnt = 0;
    double sl = 0.0, sw = 0.0;
    for (int k = tid; k < items; k += TE_NT) {
        int a = k, n;
        if (A.ego_only && scene_span(A.ptr, k, A.NA, a, n) != 0) continue;     // (a: the ego, the scene's first agent)
        add_valid_rows(A.nrm, A.pred + (size_t)a * frames * 4, frames, A.lw, a, cnt, sl, sw);
    }
    long long tot;
    double tl, tw;
    te_row_sums(tid, cnt, sl, sw, s_cnt, s_l, s_w, tot, tl, tw);
    if (tid != 0) return;
    double mean[2], ratio[2] = {eval_nan(), eval_nan()};
    int L = 0, W = 0;
    if (grid_ratios(tot, tl, tw, map, mean, ratio)) {
        const double ql = rint(ratio[0]), qw = rint(ratio[1]);
        // (saturating: a grid the table cannot serve is reported, and refused by every scene, not sampled)
        L = (ql >= -1.0e9 && ql <= 1.0e9) ? (int)ql : -1;
        W = (qw >= -1.0e9 && qw <= 1.0e9) ? (int)qw : -1;
    }
    A.grid_i[0] = L;
    A.grid_i[1] = W;
    A.grid_i[2] = tot > 0x7fffffffll ? 0x7fffffff : (int)tot;
    A.grid_d[0] = ratio[0];
    A.grid_d[1] = ratio[1];
}

__global__ __launch_bounds__(TE_NT) void traffic_eval_kernel(TrafficEvalArgs A, StriveMap map) {
#pragma clang fp contract(off)
    __shared__ double s_red[TE_NT];
    __shared__ double s_min[4][TE_NT];
    const double kNaN = eval_nan(), kInf = __longlong_as_double(0x7ff0000000000000ll);
    // gridDim.y workgroups share a scene: the (agent, step) items of err and the wave-owned flags of veh / env are dealt out across
    // them (every item still has exactly one owner, so the outputs do not depend on gridDim.y); disp and the status belong to part 0
    const int b = blockIdx.x, part = blockIdx.y, nparts = gridDim.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = part * (TE_NT / 64) + (tid >> 6), nwaves = nparts * (TE_NT / 64);
    const int T = A.T, Tg = A.Tg, NS = A.NS;
    const bool env = (A.groups & TE_ENV) != 0;
    int a0, n, L = 0, W = 0, rows = 0;
    int st = scene_span(A.ptr, b, A.NA, a0, n, env ? A.mapix : nullptr, map.M, 3);
    if (st == 0 && env) {
        L = A.grid_i[0];
        W = A.grid_i[1];
        rows = A.grid_i[2];
        if (rows > 0 && (L < 1 || L > A.lin_max || W < 1 || W > A.lin_max)) st = 4;
    }
    if (st != 0) {
        if (tid == 0 && part == 0) A.status[b] = st;
        return;
    }

    // ---- err: sample 0 of every agent against the ground truth ----
    if (A.groups & TE_ERR) {
        for (int e = part * TE_NT + tid; e < n * Tg; e += nparts * TE_NT) {
            const int a = e / Tg, t = e - a * Tg;
            const size_t ag = (size_t)(a0 + a), o = ag * Tg + t;
            double pos = kNaN, deg = kNaN;
            if (A.vis[o] == 1.0f) {
                float g[4], p[4];
                unnorm_pose(A.nrm, A.gt + o * 6, g);
                unnorm_pose(A.nrm, A.pred + (ag * NS * T + t) * 4, p);
                pose_err(g, p, pos, deg);
                deg = deg * EVAL_DEG_PER_RAD;
            }
            A.pos_err[o] = pos;
            A.ang_err[o] = deg;
        }
    }

    // ---- disp: the ego's samples against its ground truth over the common horizon ----
    if ((A.groups & TE_DISP) && part == 0) {
        const int Tc = T < Tg ? T : Tg;
        const float* gt = A.gt + (size_t)a0 * Tg * 6;
        const float* pr = A.pred + (size_t)a0 * NS * T * 4;
        double m[4] = {kInf, kInf, kInf, kInf};
        for (int s = tid; s < NS; s += TE_NT) {
            double sd = 0.0, sa = 0.0, pos = 0.0, deg = 0.0;
            for (int t = 0; t < Tc; ++t) {
                float g[4], p[4];
                unnorm_pose(A.nrm, gt + (size_t)t * 6, g);
                unnorm_pose(A.nrm, pr + ((size_t)s * T + t) * 4, p);
                pose_err(g, p, pos, deg);
                deg = deg * EVAL_DEG_PER_RAD;
                sd += pos;
                sa += deg;
            }
            m[0] = te_min(m[0], sd / (double)Tc);
            m[1] = te_min(m[1], pos);
            m[2] = te_min(m[2], sa / (double)Tc);
            m[3] = te_min(m[3], deg);
        }
        double acc = 0.0;
        const int per = NS * Tc;
        for (int e = tid; e < NS * per; e += TE_NT) {
            const int s = e / per, r = e - s * per, s2 = r / Tc, t = r - s2 * Tc;
            if (s2 <= s) continue;
            float p[4], q[4];
            unnorm_pose(A.nrm, pr + ((size_t)s * T + t) * 4, p);
            unnorm_pose(A.nrm, pr + ((size_t)s2 * T + t) * 4, q);
            const double ex = (double)p[0] - (double)q[0], ey = (double)p[1] - (double)q[1];
            acc += sqrt(ex * ex + ey * ey);
        }
        s_red[tid] = acc;
        for (int c = 0; c < 4; ++c) s_min[c][tid] = m[c];
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int i = 0; i < TE_NT; ++i) sum += s_red[i];
            for (int c = 0; c < 4; ++c) {
                double v = s_min[c][0];
                for (int i = 1; i < TE_NT; ++i) v = te_min(v, s_min[c][i]);
                A.disp[(size_t)b * 5 + c] = v;
            }
            A.disp[(size_t)b * 5 + 4] = (2.0 * sum) / ((double)NS * (double)(NS - 1) * (double)Tc);
        }
    }

    // ---- veh: one wave per (agent, sample) flag ----
    if (A.groups & TE_VEH) {
        for (int f = wave; f < n * NS; f += nwaves) {
            const int i = f / NS, s = f - i * NS;
            const int items = (n - 1 - i) * T;
            float lwi[2];
            unnorm_lw(A.nrm, A.lw, a0 + i, lwi);
            const size_t jstride = (size_t)NS * T * 4;                       // sample s of the next agent
            const float* pi = A.pred + ((size_t)(a0 + i) * NS + s) * T * 4;
            const bool hit = wave_pair_vote<false>(A.nrm, pi, lwi, pi + jstride, jstride, A.lw + (size_t)(a0 + i + 1) * 2, items, T, lane) < items;
            if (lane == 0) A.did_veh[(size_t)(a0 + i) * NS + s] = hit ? 1 : 0;
        }
    }

    // ---- env: one wave per (agent, sample) flag, frames in order, lanes over the sampling grid ----
    if (env) {
        const int nag = A.ego_only ? 1 : n, m = A.mapix[b];
        for (int f = wave; f < nag * NS; f += nwaves) {
            const int a = f / NS, s = f - a * NS, ag = a0 + a;
            float lwa[2];
            unnorm_lw(A.nrm, A.lw, ag, lwa);
            bool hit = false;
            for (int t = 0; rows > 0 && t < T && !hit; ++t) {
                float u[4];
                unnorm_pose(A.nrm, A.pred + (((size_t)ag * NS + s) * T + t) * 4, u);
                if (nan4(u)) continue;
                hit = wave_off_road(map, m, u, lwa, A.lin_tab, L, W, lane);
            }
            if (lane == 0) A.did_map[(size_t)(A.ego_only ? b : ag) * NS + s] = hit ? 1 : 0;
        }
    }
    if (tid == 0 && part == 0) A.status[b] = 0;
}

extern "C" int strive_traffic_eval_metrics(const float* pred, const float* gt, const float* vis, const int32_t* ptr, const float* lw,
                                           const float* state_mean4_host, const float* state_std4_host,
                                           const float* att_mean2_host, const float* att_std2_host, const StriveMap* map,
                                           const int32_t* mapix, const float* lin_tab, int32_t lin_max, int32_t groups,
                                           int32_t env_ego_only, int32_t B, int32_t NA, int32_t NS, int32_t T, int32_t Tg,
                                           double* pos_err, double* ang_err, double* disp, int32_t* did_veh, int32_t* did_map,
                                           int32_t* grid_i, double* grid_d, int32_t* status, strive_stream_t stream) {
    STRIVE_CHECK_ARG(pred && ptr && lw && status, "null argument");
    TrafficEvalArgs A;
    STRIVE_CHECK_ARG(eval_norm_fill(A.nrm, state_mean4_host, state_std4_host, att_mean2_host, att_std2_host), "null normaliser statistics");
    STRIVE_CHECK_ARG((groups & ~(TE_ERR | TE_DISP | TE_VEH | TE_ENV | TE_GRID_GIVEN)) == 0, "unknown metric group");
    STRIVE_CHECK_ARG(NA >= 0 && NS >= 1 && T >= 1 && Tg >= 1, "bad sizes");
    STRIVE_CHECK_ARG((long long)NA * NS < 0x7fffffffll && (long long)NA * (T > Tg ? T : Tg) < 0x7fffffffll &&
                     (long long)NS * NS * (T < Tg ? T : Tg) < 0x7fffffffll, "sizes exceed the 32-bit item counts");
    STRIVE_CHECK_ARG(!(groups & TE_ERR) || (gt && vis && pos_err && ang_err && T == Tg), "err needs gt, vis, its outputs and T == Tg");
    STRIVE_CHECK_ARG(!(groups & TE_DISP) || (gt && disp), "disp needs gt and its output");
    STRIVE_CHECK_ARG(!(groups & TE_VEH) || did_veh, "veh needs its output");
    if (groups & TE_ENV) {
        STRIVE_CHECK_ARG(map && mapix && lin_tab && lin_max >= 1 && did_map && grid_i && grid_d, "env needs a map, mapix, the linspace table and its outputs");
        STRIVE_CHECK_ARG(eval_map_ok(map), "bad map");
    }
    if (B <= 0) return 0;
    A.pred = pred; A.gt = gt; A.vis = vis; A.ptr = ptr; A.lw = lw;
    A.mapix = mapix; A.lin_tab = lin_tab; A.lin_max = lin_max;
    A.groups = groups; A.ego_only = env_ego_only ? 1 : 0;
    A.B = B; A.NA = NA; A.NS = NS; A.T = T; A.Tg = Tg;
    A.pos_err = pos_err; A.ang_err = ang_err; A.disp = disp; A.did_veh = did_veh; A.did_map = did_map;
    A.grid_i = grid_i; A.grid_d = grid_d; A.status = status;
    StriveMap m;
    memset(&m, 0, sizeof(m));
    if (map) m = *map;
    if ((groups & TE_ENV) && !(groups & TE_GRID_GIVEN)) {
        hipLaunchKernelGGL(traffic_eval_grid_kernel, dim3(1), dim3(TE_NT), 0, (hipStream_t)stream, A, m);
        STRIVE_CHECK_LAUNCH();
    }
    // latency-bound: a scene's wave-owned flags (n x NS of them) spread over up to 8 workgroups
    const int parts = NS >= 15 ? 8 : (NS >= 2 ? (NS + 1) / 2 : 1);
    hipLaunchKernelGGL(traffic_eval_kernel, dim3(B, parts), dim3(TE_NT), 0, (hipStream_t)stream, A, m);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// =============================================================================================
// Collision verdicts of the refine driver (reference src/refine_traffic_optim.py:84-121, compute_metrics) for B scenes in one host
// call without a host synchronisation, each scene as if compute_metrics had been called on that scene alone.  traj (NA,T,4) and
// lw (NA,2) arrive NORMALISED and are unnormalised in fp32 as in strive_traffic_eval_metrics (unnorm1); everything after that is
// float64.  Two launches:
//   refine_grid_kernel, one workgroup per scene: the scene's status and ITS OWN sampling grid (check_on_layer, reference
//        src/datasets/nuscenes_utils.py:266-298, forms L = round(mean_l / mean(dx)), W likewise, from the rows of one call, and the
//        reference calls it per scene): thread t counts the valid frames of the agents t, t + 256, ... in that order and adds
//        count * size (add_valid_rows), thread 0 adds the 256 partial sums in thread order (te_row_sums) and forms the grid
//        (sample_grid).  A scene without a valid row has no grid:
//        L = W = 0, ratios NaN, no environment collision.  It also writes the scene's row of out_i with both counts 0 and success 1.
//   refine_verdict_kernel, gridDim.y workgroups per scene: ONE WAVE owns a flag.
//        did_veh[i] (check_pairwise_veh_coll, reference src/losses/adv_gen_nusc.py:567-623): agent i overlaps (IoU > 0.02) some
//        agent j > i of its scene at some step; a frame with a NaN in either pose is no hit.  The reference's early exits make
//        coll_count the number of set flags, and the set does not depend on the order of evaluation: the lanes stride over (j, t),
//        reject by centre distance (boxes_apart), clip the rest (boxes_hit) and vote (wave_pair_vote).
//        did_env[a] (compute_coll_rate_env, reference src/losses/traffic_model.py:366-419): some valid frame has fp32(count) /
//        fp32(L W) < fp32(0.95) on raster layer 0; the wave walks the frames in order, its lanes stride over the L x W samples and
//        add their integer counts (wave_off_road).
//        Lane 0 writes the flag and, for a set flag, adds 1 to the scene's count and clears its success: integer atomics only, so
//        a scene's outputs are bit-identical whatever else is in the batch and however many workgroups serve the scene.
//   out_i (B,8): num_coll_veh, num_traj_veh (= n), env_coll, env_total (= n), success, L, W, valid rows (clamped to int32)
//   grid_d (B,2): the two ratios before rounding
//   status (B): 0 written; 2 offsets leave the arrays or n < 1; 3 map index out of range; 4 THIS scene's grid is outside
//        1..lin_max along an axis.  Every output of a scene with a non-zero status is untouched.
// =============================================================================================
#define RV_NI 8

struct RefineVerdictArgs {
    const float* traj; const int32_t* ptr; const float* lw;
    EvalNorm nrm;
    const int32_t* mapix; const float* lin_tab; int lin_max;
    int NA, T;
    int32_t* did_veh; int32_t* did_env; int32_t* out_i; double* grid_d; int32_t* status;
};

__global__ __launch_bounds__(TE_NT) void refine_grid_kernel(RefineVerdictArgs A, StriveMap map) {
#pragma clang fp contract(off)
    __shared__ long long s_cnt[TE_NT];
    __shared__ double s_l[TE_NT], s_w[TE_NT];
    const int b = blockIdx.x, tid = threadIdx.x, T = A.T;
    int a0, n;
    const int st = scene_span(A.ptr, b, A.NA, a0, n, A.mapix, map.M, 3);
    if (st != 0) {                                           // (uniform over the workgroup: nobody reaches the barrier below)
        if (tid == 0) A.status[b] = st;
        return;
    }
    long long cnt = 0;
    double sl = 0.0, sw = 0.0;
    for (int a = tid; a < n; a += TE_NT) add_valid_rows(A.nrm, A.traj + (size_t)(a0 + a) * T * 4, T, A.lw, a0 + a, cnt, sl, sw);
    long long tot;
    double tl, tw;
    te_row_sums(tid, cnt, sl, sw, s_cnt, s_l, s_w, tot, tl, tw);
    if (tid != 0) return;
    double mean[2], ratio[2] = {eval_nan(), eval_nan()};
    int L, W;
    if (!sample_grid(tot, tl, tw, map, A.lin_max, mean, ratio, L, W)) {
        A.status[b] = 4;
        return;
    }
    int32_t* oi = A.out_i + (size_t)b * RV_NI;
    oi[0] = 0;
    oi[1] = n;
    oi[2] = 0;
    oi[3] = n;
    oi[4] = 1;
    oi[5] = L;
    oi[6] = W;
    oi[7] = tot > 0x7fffffffll ? 0x7fffffff : (int)tot;
    A.grid_d[(size_t)b * 2 + 0] = ratio[0];
    A.grid_d[(size_t)b * 2 + 1] = ratio[1];
    A.status[b] = 0;
}

__global__ __launch_bounds__(TE_NT) void refine_verdict_kernel(RefineVerdictArgs A, StriveMap map) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, T = A.T;
    const int wave = blockIdx.y * (TE_NT / 64) + (tid >> 6), nwaves = gridDim.y * (TE_NT / 64);
    if (A.status[b] != 0) return;                            // (refine_grid_kernel checked the offsets and the map index)
    const int a0 = A.ptr[b], n = A.ptr[b + 1] - a0;
    int32_t* oi = A.out_i + (size_t)b * RV_NI;

    // ---- veh: one wave per agent flag ----
    for (int i = wave; i < n; i += nwaves) {
        const int items = (n - 1 - i) * T;
        float lwi[2];
        unnorm_lw(A.nrm, A.lw, a0 + i, lwi);
        const float* pi = A.traj + (size_t)(a0 + i) * T * 4;
        const size_t jstride = (size_t)T * 4;
        const bool hit = wave_pair_vote<true>(A.nrm, pi, lwi, pi + jstride, jstride, A.lw + (size_t)(a0 + i + 1) * 2, items, T, lane) < items;
        if (lane == 0) {
            A.did_veh[a0 + i] = hit ? 1 : 0;
            if (hit) {
                atomicAdd(&oi[0], 1);
                atomicExch(&oi[4], 0);
            }
        }
    }

    // ---- env: one wave per agent flag, frames in order, lanes over the scene's sampling grid ----
    const int L = oi[5], W = oi[6], m = A.mapix[b], cells = L * W;
    for (int a = wave; a < n; a += nwaves) {
        float lwa[2];
        unnorm_lw(A.nrm, A.lw, a0 + a, lwa);
        bool hit = false;
        for (int t = 0; cells > 0 && t < T && !hit; ++t) {
            float u[4];
            unnorm_pose(A.nrm, A.traj + ((size_t)(a0 + a) * T + t) * 4, u);
            if (nan4(u)) continue;
            hit = wave_off_road(map, m, u, lwa, A.lin_tab, L, W, lane);
        }
        if (lane == 0) {
            A.did_env[a0 + a] = hit ? 1 : 0;
            if (hit) {
                atomicAdd(&oi[2], 1);
                atomicExch(&oi[4], 0);
            }
        }
    }
}

extern "C" int strive_refine_verdicts(const float* traj, const int32_t* ptr, const float* lw, const float* state_mean4_host,
                                      const float* state_std4_host, const float* att_mean2_host, const float* att_std2_host,
                                      const StriveMap* map, const int32_t* mapix, const float* lin_tab, int32_t lin_max, int32_t B,
                                      int32_t NA, int32_t T, int32_t* did_veh, int32_t* did_env, int32_t* out_i, double* grid_d,
                                      int32_t* status, strive_stream_t stream) {
    STRIVE_CHECK_ARG(traj && ptr && lw && did_veh && did_env && out_i && grid_d && status, "null argument");
    RefineVerdictArgs A;
    STRIVE_CHECK_ARG(eval_norm_fill(A.nrm, state_mean4_host, state_std4_host, att_mean2_host, att_std2_host), "null normaliser statistics");
    STRIVE_CHECK_ARG(map && mapix && lin_tab && lin_max >= 1, "the verdicts need a map, mapix and the linspace table");
    STRIVE_CHECK_ARG(eval_map_ok(map), "bad map");
    STRIVE_CHECK_ARG(NA >= 0 && T >= 1 && (long long)NA * T < 0x7fffffffll, "bad sizes");
    if (B <= 0) return 0;
    A.traj = traj; A.ptr = ptr; A.lw = lw;
    A.mapix = mapix; A.lin_tab = lin_tab; A.lin_max = lin_max;
    A.NA = NA; A.T = T;
    A.did_veh = did_veh; A.did_env = did_env; A.out_i = out_i; A.grid_d = grid_d; A.status = status;
    hipLaunchKernelGGL(refine_grid_kernel, dim3(B), dim3(TE_NT), 0, (hipStream_t)stream, A, *map);
    STRIVE_CHECK_LAUNCH();
    // latency-bound like traffic_eval_kernel: a scene's 2 n wave-owned flags spread over up to 8 workgroups of 4 waves, by the
    // mean scene size (the host holds no per-scene count)
    const int flags = 2 * ((NA + B - 1) / B);
    const int want = (flags + 3) / 4, parts = want < 1 ? 1 : (want > 8 ? 8 : want);
    hipLaunchKernelGGL(refine_verdict_kernel, dim3(B, parts), dim3(TE_NT), 0, (hipStream_t)stream, A, *map);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// =============================================================================================
// Ego-against-others verdicts of the scenario generator (check_single_veh_coll, reference src/losses/adv_gen_nusc.py:517-565, as
// compute_adv_gen_success, reference src/utils/adv_gen_optim.py:214-235, and compute_sol_success, reference
// src/utils/sol_optim.py:126-165, call it) for B scenes in one launch without a host synchronisation, each scene as if judged
// alone.  traj (NA,T,4) and lw (NA,2) arrive NORMALISED and are unnormalised in fp32 (unnorm1); everything after that is float64.
// One workgroup of EV_NW waves per scene:
//   thread 0 forms the scene's status and, if asked, the sampling grid of ITS ego rows alone (compute_coll_rate_env with
//        ego_only=True on a single scene hands check_on_layer the ego's valid frames and nothing else: valid_frames, sample_grid);
//   wave w owns the other agents 1 + w, 1 + w + EV_NW, ...: its lanes take the steps in order, 64 at a time, reject by centre distance
//        (boxes_apart), clip the rest (boxes_hit) and vote; the lowest set lane of the first non-empty vote is the collision step
//        (wave_pair_vote with one other agent);
//   wave w owns the ego frames w, w + EV_NW, ... of the drivable test, its lanes stride over the L x W samples (integer counts:
//        wave_off_road);
//   thread 0 adds the waves' integer counts in wave order.  No atomics at all.
//   hit (NA), coll_t (NA): per other agent; the ego's row holds the scene's own n_hit > 0 and first_t
//   out_i (B,8): n_others, n_hit, atk_hit (-1 without an attacker), first_t (T if none), ego_env (-1 if not asked), L, W, valid ego rows
//   grid_d (B,2): the two ratios before rounding (NaN if not asked or without a valid ego row)
//   status (B): 0 written; 2 offsets leave the arrays, n < 1 or an attacker index other than -1 outside 1..n-1; 3 map index out of
//        range; 4 the scene's grid is outside 1..lin_max.  Every output of a scene with a non-zero status is untouched.
// =============================================================================================
#define EV_NI 8
#define EV_NW (TE_NT / 64)

struct EgoVerdictArgs {
    const float* traj; const int32_t* ptr; const float* lw; const int32_t* atk;
    EvalNorm nrm;
    const int32_t* mapix; const float* lin_tab; int lin_max, want_env;
    int NA, T;
    int32_t* hit; int32_t* coll_t; int32_t* out_i; double* grid_d; int32_t* status;
};

__global__ __launch_bounds__(TE_NT) void ego_verdict_kernel(EgoVerdictArgs A, StriveMap map) {
#pragma clang fp contract(off)
    __shared__ int s_grid[4], s_atk, s_hit[EV_NW], s_first[EV_NW], s_env[EV_NW];
    __shared__ double s_ratio[2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = A.T;
    const int atk = A.atk ? A.atk[b] : -1;
    int a0, n;
    int st = scene_span(A.ptr, b, A.NA, a0, n, A.want_env ? A.mapix : nullptr, map.M, 3);
    if (st != 2 && atk != -1 && (atk < 1 || atk >= n)) st = 2;        // (a bad attacker index goes before a bad map index)
    if (st != 0) {                                           // (uniform over the workgroup: nobody reaches the barriers below)
        if (tid == 0) A.status[b] = st;
        return;
    }
    float lwe[2];
    unnorm_lw(A.nrm, A.lw, a0, lwe);
    const float* pe = A.traj + (size_t)a0 * T * 4;
    if (tid == 0) {
        int L = 0, W = 0, rows = 0, bad = 0;
        double mean[2], ratio[2] = {eval_nan(), eval_nan()};
        if (A.want_env) {
            rows = valid_frames(A.nrm, pe, T);
            bad = sample_grid(rows, (double)rows * (double)lwe[0], (double)rows * (double)lwe[1], map, A.lin_max, mean, ratio, L, W) ? 0 : 1;
        }
        s_grid[0] = bad; s_grid[1] = L; s_grid[2] = W; s_grid[3] = rows;
        s_ratio[0] = ratio[0]; s_ratio[1] = ratio[1];
        s_atk = -1;
    }
    __syncthreads();
    if (s_grid[0] != 0) {
        if (tid == 0) A.status[b] = 4;
        return;
    }

    // ---- the ego against each other agent: one wave per agent, the steps in order ----
    int cnt = 0, first = T;
    for (int j = 1 + wave; j < n; j += EV_NW) {
        // (wave_pair_vote with ONE other agent: its T items are the steps, so the item it returns is the step of the first contact)
        const int ct = wave_pair_vote<true>(A.nrm, pe, lwe, A.traj + (size_t)(a0 + j) * T * 4, 0, A.lw + (size_t)(a0 + j) * 2, T, T, lane);
        cnt += ct < T ? 1 : 0;
        first = ct < first ? ct : first;
        if (lane == 0) {
            A.hit[a0 + j] = ct < T ? 1 : 0;
            A.coll_t[a0 + j] = ct;
            if (j == atk) s_atk = ct < T ? 1 : 0;
        }
    }

    // ---- the ego on the drivable area: one wave per frame, lanes over the scene's sampling grid ----
    const int L = s_grid[1], W = s_grid[2], cells = L * W;
    int env = 0;
    if (A.want_env && cells > 0) {
        const int m = A.mapix[b];
        for (int t = wave; t < T && !env; t += EV_NW) {
            float u[4];
            unnorm_pose(A.nrm, pe + (size_t)t * 4, u);
            if (nan4(u)) continue;
            env = wave_off_road(map, m, u, lwe, A.lin_tab, L, W, lane) ? 1 : 0;
        }
    }
    if (lane == 0) {
        s_hit[wave] = cnt;
        s_first[wave] = first;
        s_env[wave] = env;
    }
    __syncthreads();
    if (tid != 0) return;
    int n_hit = 0, first_t = T, ego_env = 0;
    for (int w = 0; w < EV_NW; ++w) {
        n_hit += s_hit[w];
        first_t = s_first[w] < first_t ? s_first[w] : first_t;
        ego_env |= s_env[w];
    }
    int32_t* oi = A.out_i + (size_t)b * EV_NI;
    oi[0] = n - 1;
    oi[1] = n_hit;
    oi[2] = atk == -1 ? -1 : s_atk;
    oi[3] = first_t;
    oi[4] = A.want_env ? ego_env : -1;
    oi[5] = L;
    oi[6] = W;
    oi[7] = s_grid[3];
    A.grid_d[(size_t)b * 2 + 0] = s_ratio[0];
    A.grid_d[(size_t)b * 2 + 1] = s_ratio[1];
    A.hit[a0] = n_hit > 0 ? 1 : 0;
    A.coll_t[a0] = first_t;
    A.status[b] = 0;
}

extern "C" int strive_ego_verdicts(const float* traj, const int32_t* ptr, const float* lw, const int32_t* atk,
                                   const float* state_mean4_host, const float* state_std4_host, const float* att_mean2_host,
                                   const float* att_std2_host, int32_t want_env, const StriveMap* map, const int32_t* mapix,
                                   const float* lin_tab, int32_t lin_max, int32_t B, int32_t NA, int32_t T, int32_t* hit,
                                   int32_t* coll_t, int32_t* out_i, double* grid_d, int32_t* status, strive_stream_t stream) {
    STRIVE_CHECK_ARG(traj && ptr && lw && hit && coll_t && out_i && grid_d && status, "null argument");
    EgoVerdictArgs A;
    STRIVE_CHECK_ARG(eval_norm_fill(A.nrm, state_mean4_host, state_std4_host, att_mean2_host, att_std2_host), "null normaliser statistics");
    STRIVE_CHECK_ARG(!want_env || (map && mapix && lin_tab && lin_max >= 1), "want_env needs a map, mapix and the linspace table");
    STRIVE_CHECK_ARG(!want_env || eval_map_ok(map), "bad map");
    STRIVE_CHECK_ARG(NA >= 0 && T >= 1 && (long long)NA * T < 0x7fffffffll, "bad sizes");
    if (B <= 0) return 0;
    A.traj = traj; A.ptr = ptr; A.lw = lw; A.atk = atk;
    A.mapix = mapix; A.lin_tab = lin_tab; A.lin_max = lin_max; A.want_env = want_env ? 1 : 0;
    A.NA = NA; A.T = T;
    A.hit = hit; A.coll_t = coll_t; A.out_i = out_i; A.grid_d = grid_d; A.status = status;
    StriveMap none = {};
    hipLaunchKernelGGL(ego_verdict_kernel, dim3(B), dim3(TE_NT), 0, (hipStream_t)stream, A, want_env ? *map : none);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// =============================================================================================
// Feasibility screening of the scenario generator (determine_feasibility_nusc, reference src/utils/scenario_gen.py:30-107, with
// check_line_layer, reference src/datasets/nuscenes_utils.py:300-332, and the two ego-speed rules of reference
// src/adv_scenario_gen.py:176-195) for B scenes in one launch without a host synchronisation, each scene as if screened alone.
// samples (NA,NS,FT,4) and gt (NA,Tg,4) arrive NORMALISED and are unnormalised in fp32 (unnorm1); distances, cosines, speeds and
// line lengths are float64 on those fp32 values; the line samples are fp32, operation for operation (fs_line_weight).
// One workgroup of FS_NW waves per scene, a wave per non-ego agent (fs_agent: lanes over the steps, the samples of a step in order,
// then a lexicographic (distance, step) butterfly, so the first sample and the first step win a tie).  The kernel keeps nothing per
// agent between its phases: it walks the agents up to three times and forms the same values each time.
//   pass 0: the scene's own line length sep_n = max over ITS agents of rint(|agent - ego| / mean(dx)) (check_line_layer takes the
//           maximum over the rows of one call, and the reference calls it per scene)
//   pass 1: (check_sep only) does any line sample leave the raster -> status 6, nothing written
//   pass 2: the lines again, the outputs per agent, and the scene's counts, which thread 0 adds in wave order
// No atomics at all, every reduction in a fixed order or order-free (integer sums, lexicographic minima, maxima without NaN).
//   per non-ego agent (the ego's rows are untouched): feasible, within, step, best_samp, sep_zero int32; dist, max_vel double
//   out_i (B,8): n_others, n_within, n_feasible_any_category, n_feasible, heur_agt (local index, -1 if none), heur_t (-1 if none),
//        sep_n, verdict (1 ego too slow, 2 ego only, 3 no vehicle near, 4 none of the requested category, 0 feasible)
//   out_d (B,3): largest ego step displacement over the samples, the same over gt's ego row (NaN without gt or with Tg < 2; a NaN
//        in gt gives NaN), heur_dist (inf if none)
//   status (B): 0 written; 2 offsets leave the arrays or n < 1; 3 map index out of range; 5 a sample that is not finite after
//        unnormalising; 6 a line sample outside the raster, or sep_n above FS_LINE_MAX.  Nothing of such a scene is written.
// =============================================================================================
#define FS_NI 8
#define FS_ND 3
#define FS_NW (TE_NT / 64)
#define FS_LINE_MAX 65536
#define FS_NO_STEP 0x7fffffff

struct FeasScreenArgs {
    const float* samples; const int32_t* ptr; const int32_t* mapix; const int32_t* allowed; const float* gt;
    EvalNorm nrm;             // (sizes are not read: the attribute half holds the identity)
    double thresh, agent_vel, ego_vel, infront_min;
    int t0, use_infront, check_sep, planner_rule;
    int NA, NS, FT, Tg;
    int32_t* feasible; int32_t* within; int32_t* step; int32_t* best_samp; int32_t* sep_zero;
    double* dist; double* max_vel; int32_t* out_i; double* out_d; int32_t* status;
};

struct FsBest {
    double dist, vel;        // closest approach after the in-front mask (inf if every step is masked); largest step displacement
    int step, samp, within;  // where it is attained (t0, 0 if every step is masked); some distance < thresh
};

__device__ __forceinline__ double fs_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// unnormalised position (and, for the ego, heading) of sample s, step t of the agent whose samples start at p
__device__ __forceinline__ void fs_xy(const FeasScreenArgs& A, const float* p, int s, int t, float& x, float& y) {
    const float* q = p + ((size_t)s * A.FT + t) * 4;
    x = unnorm1(q[0], A.nrm.sm[0], A.nrm.ss[0]);
    y = unnorm1(q[1], A.nrm.sm[1], A.nrm.ss[1]);
}

// |a - b| of two fp32 points in float64
__device__ __forceinline__ double fs_len(float ax, float ay, float bx, float by) {
#pragma clang fp contract(off)
    const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by;
    return sqrt(dx * dx + dy * dy);
}

// One non-ego agent by one wave; every lane returns the same values.
__device__ __forceinline__ FsBest fs_agent(const FeasScreenArgs& A, const float* ego, const float* agt, int lane) {
#pragma clang fp contract(off)
    const int NS = A.NS, FT = A.FT;
    double bd = fs_inf();
    int bt = FS_NO_STEP, bs = 0, within = 0;
    for (int t = A.t0 + lane; t < FT; t += 64) {
        double sd = fs_inf();
        int ssamp = 0;
        for (int s = 0; s < NS; ++s) {
            float ex, ey, ax, ay;
            fs_xy(A, ego, s, t, ex, ey);
            fs_xy(A, agt, s, t, ax, ay);
            double d = fs_len(ax, ay, ex, ey);
            if (A.use_infront) {
                const float* q = ego + ((size_t)s * FT + t) * 4;
                const double hx = (double)unnorm1(q[2], A.nrm.sm[2], A.nrm.ss[2]), hy = (double)unnorm1(q[3], A.nrm.sm[3], A.nrm.ss[3]);
                const double ux = ((double)ax - (double)ex) / d, uy = ((double)ay - (double)ey) / d;
                const double cossim = ux * hx + uy * hy;
                if (!(cossim >= A.infront_min)) d = fs_inf();            // (coincident positions: 0 / 0, not in front)
            }
            within |= d < A.thresh ? 1 : 0;
            if (d < sd) { sd = d; ssamp = s; }
        }
        if (sd < bd) { bd = sd; bt = t; bs = ssamp; }
    }
    double vel = 0.0;
    const int items = NS * (FT - 1);
    for (int e = lane; e < items; e += 64) {
        const int s = e / (FT - 1), t = e - s * (FT - 1);
        float x0, y0, x1, y1;
        fs_xy(A, agt, s, t, x0, y0);
        fs_xy(A, agt, s, t + 1, x1, y1);
        const double v = fs_len(x1, y1, x0, y0);
        vel = v > vel ? v : vel;
    }
    for (int k = 32; k >= 1; k >>= 1) {
        const double od = __shfl_xor(bd, k), ov = __shfl_xor(vel, k);
        const int ot = __shfl_xor(bt, k), os = __shfl_xor(bs, k);
        if (od < bd || (od == bd && ot < bt)) { bd = od; bt = ot; bs = os; }
        vel = ov > vel ? ov : vel;
    }
    FsBest r;
    r.dist = bd;
    r.vel = vel;
    r.step = bt == FS_NO_STEP ? A.t0 : bt;
    r.samp = bt == FS_NO_STEP ? 0 : bs;
    r.within = __ballot(within) != 0ull ? 1 : 0;
    return r;
}

// torch.linspace(0, 1, n)[i] in fp32 (n >= 1): step = 1 / (n - 1); the first half counts up from 0, the second down from 1
__device__ __forceinline__ float fs_line_weight(int i, int n) {
    if (n < 2) return 0.0f;
    const float step = __fdiv_rn(1.0f, (float)(n - 1));
    return i < n / 2 ? __fmul_rn(step, (float)i) : __fsub_rn(1.0f, __fmul_rn(step, (float)(n - 1 - i)));
}

// The n samples start * (1 - w) + end * w of one line by one wave: how many lie on a 0 pixel of the frame's layer 0, and whether
// any lies outside the raster (such a sample is not read).  Every lane returns the same values.
__device__ __forceinline__ void fs_line(const CropFrame& fr, float sx, float sy, float ex, float ey, int n, int lane, int& zero, int& outside) {
    int z = 0, o = 0;
    for (int i = lane; i < n; i += 64) {
        const float w = fs_line_weight(i, n), w1 = __fsub_rn(1.0f, w);
        const float gx = __fadd_rn(__fmul_rn(sx, w1), __fmul_rn(ex, w));
        const float gy = __fadd_rn(__fmul_rn(sy, w1), __fmul_rn(ey, w));
        const double qx = quotient_rint((double)gx, fr.dx0, fr.inv0), qy = quotient_rint((double)gy, fr.dx1, fr.inv1);
        if (qx >= 0.0 && qx < (double)fr.W && qy >= 0.0 && qy < (double)fr.H) z += fr.base[(size_t)(int)qy * fr.W + (int)qx] == 0 ? 1 : 0;
        else o = 1;
    }
    for (int k = 32; k >= 1; k >>= 1) z += __shfl_xor(z, k);
    zero = z;
    outside = __ballot(o) != 0ull ? 1 : 0;
}

__global__ __launch_bounds__(TE_NT) void feasibility_screen_kernel(FeasScreenArgs A, StriveMap map) {
#pragma clang fp contract(off)
    __shared__ int s_bad[FS_NW], s_n[FS_NW], s_out[FS_NW], s_cnt[FS_NW][3], s_ha[FS_NW], s_ht[FS_NW];
    __shared__ double s_ev[FS_NW], s_hd[FS_NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NS = A.NS, FT = A.FT;
    int a0, n;
    const int st = scene_span(A.ptr, b, A.NA, a0, n, A.mapix, map.M, 3);
    if (st != 0) {                                           // (uniform over the workgroup: nobody reaches the barriers below)
        if (tid == 0) A.status[b] = st;
        return;
    }
    const float* ego = A.samples + (size_t)a0 * NS * FT * 4;

    // ---- every sample of the scene is finite; the ego's largest step displacement over its samples ----
    int bad = 0;
    const size_t vals = (size_t)n * NS * FT * 4;
    for (size_t i = tid; i < vals; i += TE_NT) {
        const int c = (int)(i & 3);
        bad |= fabsf(unnorm1(ego[i], A.nrm.sm[c], A.nrm.ss[c])) <= 3.4028234663852886e38f ? 0 : 1;
    }
    double ev = 0.0;
    for (int e = tid; e < NS * (FT - 1); e += TE_NT) {
        const int s = e / (FT - 1), t = e - s * (FT - 1);
        float x0, y0, x1, y1;
        fs_xy(A, ego, s, t, x0, y0);
        fs_xy(A, ego, s, t + 1, x1, y1);
        const double v = fs_len(x1, y1, x0, y0);
        ev = v > ev ? v : ev;
    }
    for (int k = 32; k >= 1; k >>= 1) {
        const double ov = __shfl_xor(ev, k);
        ev = ov > ev ? ov : ev;
    }
    bad = __ballot(bad) != 0ull ? 1 : 0;
    if (lane == 0) {
        s_bad[wave] = bad;
        s_ev[wave] = ev;
    }
    __syncthreads();
    bad = 0;
    ev = 0.0;
    for (int w = 0; w < FS_NW; ++w) {
        bad |= s_bad[w];
        ev = s_ev[w] > ev ? s_ev[w] : ev;
    }
    if (bad) {
        if (tid == 0) A.status[b] = 5;
        return;
    }

    double sdx = 0.0;
    for (int m = 0; m < map.M * 2; ++m) sdx += map.dx[m];
    const double mdx = sdx / (double)(map.M * 2);
    float zero4[4] = {0.0f, 0.0f, 1.0f, 0.0f};
    const CropFrame fr = map_frame(map, A.mapix[b], zero4);

    int sep_n = 0;
    int n_within = 0, n_any = 0, n_feas = 0, ha = -1, ht = -1;
    double hd = fs_inf();
    for (int pass = 0; pass < 3; ++pass) {
        if (pass == 1 && !A.check_sep) continue;
        int wn = 0, wout = 0;
        for (int j = 1 + wave; j < n; j += FS_NW) {
            const float* agt = A.samples + (size_t)(a0 + j) * NS * FT * 4;
            const FsBest r = fs_agent(A, ego, agt, lane);
            float ax, ay, ex, ey;
            fs_xy(A, agt, r.samp, r.step, ax, ay);
            fs_xy(A, ego, r.samp, r.step, ex, ey);
            if (pass == 0) {
                const double q = rint(fs_len(ax, ay, ex, ey) / mdx);
                const int na = q <= (double)FS_LINE_MAX ? (int)q : FS_LINE_MAX + 1;
                wn = na > wn ? na : wn;
                continue;
            }
            int zero = 0, outside = 0;
            if (A.check_sep) fs_line(fr, ax, ay, ex, ey, sep_n, lane, zero, outside);
            wout |= outside;
            if (pass == 1) continue;
            const int any = (r.within && zero == 0 && r.vel > A.agent_vel) ? 1 : 0;
            const int feas = (any && (!A.allowed || A.allowed[a0 + j] != 0)) ? 1 : 0;
            n_within += r.within;
            n_any += any;
            n_feas += feas;
            if (feas && (r.dist < hd || (r.dist == hd && j < ha))) { hd = r.dist; ha = j; ht = r.step; }
            if (lane == 0) {
                A.feasible[a0 + j] = feas;
                A.within[a0 + j] = r.within;
                A.step[a0 + j] = r.step;
                A.best_samp[a0 + j] = r.samp;
                A.sep_zero[a0 + j] = zero;
                A.dist[a0 + j] = r.dist;
                A.max_vel[a0 + j] = r.vel;
            }
        }
        if (pass == 0) {
            if (lane == 0) s_n[wave] = wn;
            __syncthreads();
            for (int w = 0; w < FS_NW; ++w) sep_n = s_n[w] > sep_n ? s_n[w] : sep_n;
            if (sep_n > FS_LINE_MAX) {
                if (tid == 0) A.status[b] = 6;
                return;
            }
        } else if (pass == 1) {
            if (lane == 0) s_out[wave] = wout;
            __syncthreads();
            wout = 0;
            for (int w = 0; w < FS_NW; ++w) wout |= s_out[w];
            if (wout) {
                if (tid == 0) A.status[b] = 6;
                return;
            }
        }
    }
    if (lane == 0) {
        s_cnt[wave][0] = n_within; s_cnt[wave][1] = n_any; s_cnt[wave][2] = n_feas;
        s_ha[wave] = ha; s_ht[wave] = ht; s_hd[wave] = hd;
    }
    __syncthreads();
    if (tid != 0) return;
    n_within = n_any = n_feas = 0;
    ha = ht = -1;
    hd = fs_inf();
    for (int w = 0; w < FS_NW; ++w) {
        n_within += s_cnt[w][0];
        n_any += s_cnt[w][1];
        n_feas += s_cnt[w][2];
        if (s_ha[w] >= 0 && (s_hd[w] < hd || (s_hd[w] == hd && s_ha[w] < ha))) { hd = s_hd[w]; ha = s_ha[w]; ht = s_ht[w]; }
    }
    // the ego's largest step displacement over gt's ego row, as torch.max gives it: a NaN wins
    double gv = eval_nan();
    if (A.gt && A.Tg >= 2) {
        const float* g = A.gt + (size_t)a0 * A.Tg * 4;
        gv = 0.0;
        for (int t = 0; t + 1 < A.Tg; ++t) {
            const float x0 = unnorm1(g[t * 4 + 0], A.nrm.sm[0], A.nrm.ss[0]), y0 = unnorm1(g[t * 4 + 1], A.nrm.sm[1], A.nrm.ss[1]);
            const float x1 = unnorm1(g[t * 4 + 4], A.nrm.sm[0], A.nrm.ss[0]), y1 = unnorm1(g[t * 4 + 5], A.nrm.sm[1], A.nrm.ss[1]);
            const double v = fs_len(x1, y1, x0, y0);
            gv = (gv != gv || v != v) ? (gv + v) : (v > gv ? v : gv);
        }
    }
    const double ego_v = A.planner_rule == 1 ? gv : ev;
    const bool slow = A.planner_rule != 0 && ego_v < A.ego_vel;
    int32_t* oi = A.out_i + (size_t)b * FS_NI;
    oi[0] = n - 1;
    oi[1] = n_within;
    oi[2] = n_any;
    oi[3] = n_feas;
    oi[4] = ha;
    oi[5] = ht;
    oi[6] = sep_n;
    oi[7] = slow ? 1 : (n == 1 ? 2 : (n_any == 0 ? 3 : (n_feas == 0 ? 4 : 0)));
    double* od = A.out_d + (size_t)b * FS_ND;
    od[0] = ev;
    od[1] = gv;
    od[2] = hd;
    A.status[b] = 0;
}

extern "C" int strive_feasibility_screen(const float* samples, const int32_t* ptr, const int32_t* mapix, const int32_t* allowed,
                                         const float* gt, const float* state_mean4_host, const float* state_std4_host,
                                         const StriveMap* map, double thresh, int32_t t0, double agent_vel, double ego_vel,
                                         int32_t use_infront, double infront_min, int32_t check_sep, int32_t planner_rule, int32_t B,
                                         int32_t NA, int32_t NS, int32_t FT, int32_t Tg, int32_t* feasible, int32_t* within,
                                         int32_t* step, int32_t* best_samp, double* dist, int32_t* sep_zero, double* max_vel,
                                         int32_t* out_i, double* out_d, int32_t* status, strive_stream_t stream) {
    STRIVE_CHECK_ARG(samples && ptr && mapix && feasible && within && step && best_samp && dist && sep_zero && max_vel, "null argument");
    STRIVE_CHECK_ARG(out_i && out_d && status && state_mean4_host && state_std4_host, "null argument");
    STRIVE_CHECK_ARG(eval_map_ok(map), "bad map");
    STRIVE_CHECK_ARG(NA >= 0 && NS >= 1 && FT >= 2 && (long long)NA * NS * FT < 0x1fffffffll, "bad sizes");
    STRIVE_CHECK_ARG(t0 >= 0 && t0 < FT, "feasibility_time outside the horizon");
    STRIVE_CHECK_ARG(!use_infront || (infront_min >= -1.0 && infront_min <= 1.0), "feasibility_infront_min must lie in [-1, 1]");
    STRIVE_CHECK_ARG(planner_rule >= 0 && planner_rule <= 2, "planner_rule is 0 (none), 1 (gt) or 2 (samples)");
    STRIVE_CHECK_ARG(planner_rule != 1 || (gt && Tg >= 2), "the gt rule needs gt with at least two steps");
    STRIVE_CHECK_ARG(!gt || (Tg >= 1 && (long long)NA * Tg < 0x1fffffffll), "bad gt size");
    if (B <= 0) return 0;
    FeasScreenArgs A;
    A.samples = samples; A.ptr = ptr; A.mapix = mapix; A.allowed = allowed; A.gt = gt;
    const float att_mean[2] = {0.0f, 0.0f}, att_std[2] = {1.0f, 1.0f};
    eval_norm_fill(A.nrm, state_mean4_host, state_std4_host, att_mean, att_std);
    A.thresh = thresh; A.agent_vel = agent_vel; A.ego_vel = ego_vel; A.infront_min = infront_min;
    A.t0 = t0; A.use_infront = use_infront ? 1 : 0; A.check_sep = check_sep ? 1 : 0; A.planner_rule = planner_rule;
    A.NA = NA; A.NS = NS; A.FT = FT; A.Tg = Tg;
    A.feasible = feasible; A.within = within; A.step = step; A.best_samp = best_samp; A.sep_zero = sep_zero;
    A.dist = dist; A.max_vel = max_vel; A.out_i = out_i; A.out_d = out_d; A.status = status;
    hipLaunchKernelGGL(feasibility_screen_kernel, dim3(B), dim3(TE_NT), 0, (hipStream_t)stream, A, *map);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// =============================================================================================
// One Lloyd step of k-means on N x F float64 features (the clustering of reference src/cluster_scenarios.py, whose
// KMeans.fit / .predict run scikit-learn on the host): every row's nearest centre (squared distance summed over the
// features in order, the lowest index on equal distance), then per-cluster sums and counts and the inertia.  No atomics on
// doubles: workgroup j of the second launch owns cluster j (workgroup k the inertia), every thread adds its rows in
// ascending order and the 256 partials meet in a fixed binary tree, so two runs give the same bytes.
// =============================================================================================
#define KM_MAX_F 8
#define KM_MAX_K 64

__global__ __launch_bounds__(256) void kmeans_assign_kernel(const double* __restrict__ x, const double* __restrict__ cen, int N, int F,
                                                              int k, int32_t* __restrict__ labels, double* __restrict__ mind) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    double v[KM_MAX_F];
    for (int f = 0; f < F; ++f) v[f] = x[(size_t)r * F + f];
    double best = 0.0;
    int bj = 0;
    for (int j = 0; j < k; ++j) {
        double d = 0.0;
        for (int f = 0; f < F; ++f) {
            const double e = v[f] - cen[j * F + f];
            d += e * e;
        }
        if (j == 0 || d < best) {
            best = d;
            bj = j;
        }
    }
    labels[r] = bj;
    mind[r] = best;
}

__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const double* __restrict__ x, const int32_t* __restrict__ labels,
                                                              const double* __restrict__ mind, int N, int F, int k,
                                                              double* __restrict__ sums, int32_t* __restrict__ counts,
                                                              double* __restrict__ inertia) {
    __shared__ double s_acc[256][KM_MAX_F + 1];
    __shared__ int s_n[256];
    const int j = blockIdx.x, tid = threadIdx.x;
    double acc[KM_MAX_F] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    if (j < k) {
        for (int r = tid; r < N; r += 256)
            if (labels[r] == j) {
                for (int f = 0; f < F; ++f) acc[f] += x[(size_t)r * F + f];
                ++cnt;
            }
    } else {
        for (int r = tid; r < N; r += 256) acc[0] += mind[r];
    }
    for (int f = 0; f < KM_MAX_F; ++f) s_acc[tid][f] = acc[f];
    s_n[tid] = cnt;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            for (int f = 0; f < KM_MAX_F; ++f) s_acc[tid][f] += s_acc[tid + s][f];
            s_n[tid] += s_n[tid + s];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    if (j < k) {
        for (int f = 0; f < F; ++f) sums[j * F + f] = s_acc[0][f];
        counts[j] = s_n[0];
    } else {
        inertia[0] = s_acc[0][0];
    }
}

extern "C" int strive_kmeans_step(const double* x, const double* centers, int32_t N, int32_t F, int32_t k, int32_t* labels,
                                  double* mind, double* sums, int32_t* counts, double* inertia, strive_stream_t stream) {
    STRIVE_CHECK_ARG(x && centers && labels && mind && sums && counts && inertia, "null argument");
    STRIVE_CHECK_ARG(F >= 1 && F <= KM_MAX_F, "F must be 1..8");
    STRIVE_CHECK_ARG(k >= 1 && k <= KM_MAX_K, "k must be 1..64");
    STRIVE_CHECK_ARG(N >= 1, "N must be at least 1");
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, centers, N, F, k, labels, mind);
    STRIVE_CHECK_LAUNCH();
    hipLaunchKernelGGL(kmeans_reduce_kernel, dim3(k + 1), dim3(256), 0, (hipStream_t)stream, x, (const int32_t*)labels,
                       (const double*)mind, N, F, k, sums, counts, inertia);
    STRIVE_CHECK_LAUNCH();
    return 0;
}
