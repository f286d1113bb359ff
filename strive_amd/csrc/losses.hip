// Vehicle-vehicle collision penalty with the 5-circle approximation, forward and backward.
// (reference src/losses/adv_gen_nusc.py:405-512; training variant src/losses/traffic_model.py:166-238)
//
// The reference expands every ordered pair of the WHOLE batch at every time sample into two
// (T*NA*NA, 5, 2) tensors, runs cdist and only then masks out cross-scene pairs; here only the in-scene
// blocks exist: sum_b n_b^2 slots per time sample instead of NA^2 (32x fewer at 32 scenes of 16).
// One thread owns (agent i, time t) and walks the members j of i's scene; the scene's circle centres
// are a few hundred bytes, so everything stays in registers / L1.
#include <type_traits>
#include "common.h"

#define NCIRC 5

struct VehArgs {
    int NA, T, P;
    const int32_t* ptr;
    const int32_t* scene_of;
    const int32_t* pair_off;
    const float* traj;     // (NA, T, 4) unnormalised (x, y, hx, hy)
    const float* cent_x;   // (NA, 5)
    const float* rad;      // (NA)
    float buffer;
    int cull;              // fused AvoidCollLoss only (pen / amin stay inside the call): a pair whose vehicle centres are further apart than
                           // the circles can reach is written as hit = 0 without its 25 circle distances, pen and amin left unwritten --
                           // every consumer reads them behind hit.  Exact: the cull distance carries 1 mm of slack over the bound
    const uint8_t* alive;  // (B) or null: pairs of a scene with alive == 0 are written as "not colliding" (AdvGenLoss with a
                           // quarantined scene, StriveAdvGen.scene_alive): they then enter neither a sum, a count nor a gradient
};

// world-frame circle centres of agent a at time t: transform2frame(inverse) of (cx, 0)
// (reference src/utils/transforms.py:113-133): (c*cx + x, s*cx + y)
__device__ __forceinline__ void circle_centres(const VehArgs& a, int ag, int t, float* cx, float* cy) {
    const float* p = a.traj + ((size_t)ag * a.T + t) * 4;
    for (int k = 0; k < NCIRC; ++k) {
        const float c0 = a.cent_x[ag * NCIRC + k];
        cx[k] = p[2] * c0 + p[0];
        cy[k] = p[3] * c0 + p[1];
    }
}

// A group of VG consecutive lanes owns one (agent i, time t): lane g of the group handles the scene members
// jl = g, g + VG, ... so a 16-agent scene is one pass, and the backward reduces the group's partial gradients
// with shuffles (deterministic, no atomics).
#define VG 16

__global__ __launch_bounds__(256) void veh_coll_fwd_kernel(VehArgs a, float* __restrict__ pen, uint8_t* __restrict__ hit,
                                                             uint8_t* __restrict__ amin) {
    const int gid = (blockIdx.x * blockDim.x + threadIdx.x) / VG;
    const int sub = threadIdx.x & (VG - 1);
    if (gid >= a.NA * a.T) return;
    // agent fastest: the slots of consecutive agents at one time sample are contiguous in pen / hit / amin, so a wave's
    // stores (4 groups x 16 lanes) form one contiguous run instead of four runs P floats apart
    const int t = gid / a.NA, i = gid - t * a.NA;
    const int b = a.scene_of[i];
    const int lo = a.ptr[b], n = a.ptr[b + 1] - lo;
    float ax[NCIRC], ay[NCIRC];
    circle_centres(a, i, t, ax, ay);
    const float ri = a.rad[i];
    const size_t base = (size_t)t * a.P + a.pair_off[i];
    // how far a circle centre of agent i lies from its pose: max |offset| x |heading vector| (the interpolated headings are not unit)
    const float* pi = a.traj + ((size_t)i * a.T + t) * 4;
    float reach_i = 0.f;
    if (a.cull) {
        for (int k = 0; k < NCIRC; ++k) reach_i = fmaxf(reach_i, fabsf(a.cent_x[i * NCIRC + k]));
        reach_i *= sqrtf(pi[2] * pi[2] + pi[3] * pi[3]);
    }
    for (int jl = sub; jl < n; jl += VG) {
        const int j = lo + jl;
        if (a.cull) {
            // the refine loop's loss has no scene structure (reference refine_traffic_optim.py: all NA^2 pairs): at 512 agents in 32
            // scenes 97 % of the pairs are hundreds of metres apart
            const float* pj = a.traj + ((size_t)j * a.T + t) * 4;
            float reach_j = 0.f;
            for (int k = 0; k < NCIRC; ++k) reach_j = fmaxf(reach_j, fabsf(a.cent_x[j * NCIRC + k]));
            reach_j *= sqrtf(pj[2] * pj[2] + pj[3] * pj[3]);
            const float far = ((ri + a.rad[j]) + a.buffer) + reach_i + reach_j + 1e-3f;
            const float dxc = pi[0] - pj[0], dyc = pi[1] - pj[1];
            if (dxc * dxc + dyc * dyc > far * far * 1.00001f) {       // (NaN poses compare false and take the full path)
                hit[base + jl] = 0;
                continue;
            }
        }
        float bx[NCIRC], by[NCIRC];
        circle_centres(a, j, t, bx, by);
        // min over the 25 centre distances, first index on ties like torch.min.  The correctly rounded square root is
        // monotonic, so min sqrt(d2) = sqrt(min d2): one square root instead of 25.  Two different d2 can round to the same
        // distance, and the reference then reports the EARLIER index: the (rare) candidates within 2 ulp of the minimum are
        // re-checked with their own square root.
        float d2[NCIRC * NCIRC];
        float m2 = 3.0e38f;
#pragma unroll
        for (int p = 0; p < NCIRC; ++p)
#pragma unroll
            for (int q = 0; q < NCIRC; ++q) {
                const float dx = ax[p] - bx[q], dy = ay[p] - by[q];
                const float v = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
                d2[p * NCIRC + q] = v;
                m2 = fminf(m2, v);
            }
        const float dmin = m2 < 3.0e38f ? sqrtf(m2) : 3.0e38f;      // NaN poses: nothing compares below the sentinel
        const float thr = m2 * 1.0000005f;
        int am = NCIRC * NCIRC;
#pragma unroll
        for (int k = NCIRC * NCIRC - 1; k >= 0; --k)
            if (d2[k] <= thr && (d2[k] == m2 || sqrtf(d2[k]) == dmin)) am = k;
        if (am == NCIRC * NCIRC) am = 0;
        const float pd = (ri + a.rad[j]) + a.buffer;
        pen[base + jl] = 1.0f - dmin / pd;
        hit[base + jl] = (j != i && dmin <= pd && !(a.alive && !a.alive[b])) ? 1 : 0;
        amin[base + jl] = (uint8_t)am;
    }
}

// The float64 sums[] a fused loss call (AvoidCollLoss, AdvGenLoss: below) leaves in its workspace for its backward kernels.
// AvoidCollLoss has the first AV_TERMS; AdvGenLoss adds the planner pairs, which like them are summed over workgroup partials
// (ADV_TERMS accumulators), and two counts that its final kernel forms itself (ADV_SUMS entries).
enum LossSum {
    S_VEH, S_VEH_N,             // vehicle penalties: sum, number of colliding valid slots
    S_ENV, S_ENV_N,             // environment penalties: sum, number of rows with a collision point
    S_PRIOR, S_INIT,            // prior NLL sum, init-z sum (AdvGenLoss: re-weighted per row)
    AV_TERMS,
    S_PLAN = AV_TERMS, S_PLAN_N,    // planner-involving slots: re-weighted sum, count
    ADV_TERMS,
    S_ROWS = ADV_TERMS, S_SCENES,   // latent rows / scenes that are alive (all of them without a mask)
    ADV_SUMS,
    S_CRASH = ADV_SUMS,             // sum of the scenes' crash terms: stays inside adv_final_kernel (ADV_LOCAL values there)
    ADV_LOCAL
};

// Gradient of the masked MEAN of the penalties without a d_pen tensor (fused AvoidCollLoss): d_pen(slot) = g for the
// slots that are colliding and valid, g = d_loss * w / max(#such slots, 1) read from the forward's sums.
struct VehImplicit {
    const uint8_t* hit;       // (T,P)
    const uint8_t* valid;     // (P)
    const double* sums;       // LossSum: S_VEH_N = number of colliding valid slots (S_PLAN_N = of planner slots, see slot_ne)
    const float* d_loss;      // device scalar
    float w;
    // AdvGenLoss: slots that involve the scene's ego form a second masked mean, weighted per slot by rew of the non-ego
    // member (reference :192-204); slot_ne = that member's non-ego row, -1 for the other slots; null = one mean over all
    const int32_t* slot_ne;
    const float* rew;
    float w2;
};

// d_traj[i][t] += sum_j [ d_pen(i,j) * dpen(i,j)/dpose_i  +  d_pen(j,i) * dpen(j,i)/dpose_i ]
template <bool IMPL>
__global__ __launch_bounds__(256) void veh_coll_bwd_kernel(VehArgs a, const float* __restrict__ d_pen,
                                                             const uint8_t* __restrict__ amin, float* __restrict__ d_traj,
                                                             VehImplicit im) {
    const int gid_raw = (blockIdx.x * blockDim.x + threadIdx.x) / VG;
    const int sub = threadIdx.x & (VG - 1);
    const bool live = gid_raw < a.NA * a.T;      // whole groups are live or not; every lane stays for the shuffles
    const int gid = live ? gid_raw : 0;
    const int t = gid / a.NA, i = gid - t * a.NA;      // agent fastest (see the forward kernel)
    const int b = a.scene_of[i];
    const int lo = a.ptr[b], n = a.ptr[b + 1] - lo;
    float ax[NCIRC], ay[NCIRC];
    circle_centres(a, i, t, ax, ay);
    const float ri = a.rad[i];
    const int il = i - lo;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    float gs = 0.f, gs2 = 0.f;
    if (IMPL) {
        const double c = im.sums[S_VEH_N];
        gs = (float)((double)im.d_loss[0] * (double)im.w / (c < 1.0 ? 1.0 : c));
        if (im.slot_ne) {
            const double c2 = im.sums[S_PLAN_N];
            gs2 = (float)((double)im.d_loss[0] * (double)im.w2 / (c2 < 1.0 ? 1.0 : c2));
        }
    }
    auto slot_grad = [&](size_t s, int slot) -> float {
        if (!(im.hit[s] && im.valid[slot])) return 0.f;
        if (im.slot_ne) {
            const int ne = im.slot_ne[slot];
            if (ne >= 0) return gs2 * im.rew[ne];
        }
        return gs;
    };
    for (int jl = sub; live && jl < n; jl += VG) {
        const int j = lo + jl;
        if (j == i) continue;
        const size_t s_ij = (size_t)t * a.P + a.pair_off[i] + jl, s_ji = (size_t)t * a.P + a.pair_off[j] + il;
        const float gp_ij = IMPL ? slot_grad(s_ij, a.pair_off[i] + jl) : d_pen[s_ij];
        const float gp_ji = IMPL ? slot_grad(s_ji, a.pair_off[j] + il) : d_pen[s_ji];
        if (gp_ij == 0.f && gp_ji == 0.f) continue;            // (most pairs: the other agent's circles are not needed)
        float bx[NCIRC], by[NCIRC];
        circle_centres(a, j, t, bx, by);
        const float pd = (ri + a.rad[j]) + a.buffer;
        // pair (i, j): i is the first member
        {
            const size_t s = s_ij;
            const float gp = gp_ij;
            if (gp != 0.f) {
                const int am = amin[s];
                const int p = am / NCIRC, q = am - p * NCIRC;
                const float dx = ax[p] - bx[q], dy = ay[p] - by[q];
                const float d = sqrtf(dx * dx + dy * dy);
                if (d > 0.f) {
                    const float k = -gp / (pd * d);
                    const float gx = k * dx, gy = k * dy;
                    const float c0 = a.cent_x[i * NCIRC + p];
                    g[0] += gx; g[1] += gy; g[2] += gx * c0; g[3] += gy * c0;
                }
            }
        }
        // pair (j, i): i is the second member
        {
            const size_t s = s_ji;
            const float gp = gp_ji;
            if (gp != 0.f) {
                const int am = amin[s];
                const int p = am / NCIRC, q = am - p * NCIRC;   // p indexes j's circles, q indexes i's
                const float dx = bx[p] - ax[q], dy = by[p] - ay[q];
                const float d = sqrtf(dx * dx + dy * dy);
                if (d > 0.f) {
                    const float k = gp / (pd * d);
                    const float gx = k * dx, gy = k * dy;
                    const float c0 = a.cent_x[i * NCIRC + q];
                    g[0] += gx; g[1] += gy; g[2] += gx * c0; g[3] += gy * c0;
                }
            }
        }
    }
#pragma unroll
    for (int m = VG / 2; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] += __shfl_xor(g[k], m);
    if (live && sub == 0) {
        float* o = d_traj + ((size_t)i * a.T + t) * 4;
        for (int k = 0; k < 4; ++k) o[k] += g[k];
    }
}

static VehArgs veh_args(const StriveScenes* sc, const int32_t* pair_off, int P, const float* traj, int T,
                        const float* cent_x, const float* rad, float buffer) {
    VehArgs a;
    a.NA = sc->NA; a.T = T; a.P = P; a.ptr = sc->ptr; a.scene_of = sc->scene_of; a.pair_off = pair_off;
    a.traj = traj; a.cent_x = cent_x; a.rad = rad; a.buffer = buffer; a.alive = nullptr; a.cull = 0;
    return a;
}

static int veh_coll_fwd_masked(const StriveScenes* sc, const int32_t* pair_off, int32_t P, const float* traj, int32_t T,
                               const float* cent_x, const float* rad, float buffer, const uint8_t* scene_alive, float* pen,
                               uint8_t* hit, uint8_t* amin, strive_stream_t stream, int cull = 0) {
    STRIVE_CHECK_ARG(sc && pair_off && traj && cent_x && rad && pen && hit && amin, "null argument");
    STRIVE_CHECK_ARG(sc->NS == 1, "collision losses take one trajectory per agent");
    const long long n = (long long)sc->NA * T * VG;
    if (n <= 0) return 0;
    VehArgs a = veh_args(sc, pair_off, P, traj, T, cent_x, rad, buffer);
    a.alive = scene_alive;
    a.cull = cull;
    hipLaunchKernelGGL(veh_coll_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, pen, hit, amin);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int strive_veh_coll_fwd(const StriveScenes* sc, const int32_t* pair_off, int32_t P, const float* traj, int32_t T,
                                   const float* cent_x, const float* rad, float buffer, float* pen, uint8_t* hit,
                                   uint8_t* amin, strive_stream_t stream) {
    return veh_coll_fwd_masked(sc, pair_off, P, traj, T, cent_x, rad, buffer, nullptr, pen, hit, amin, stream);
}

extern "C" int strive_veh_coll_bwd(const StriveScenes* sc, const int32_t* pair_off, int32_t P, const float* traj, int32_t T,
                                   const float* cent_x, const float* rad, float buffer, const float* d_pen,
                                   const uint8_t* amin, float* d_traj, strive_stream_t stream) {
    STRIVE_CHECK_ARG(sc && pair_off && traj && cent_x && rad && d_pen && amin && d_traj, "null argument");
    STRIVE_CHECK_ARG(sc->NS == 1, "collision losses take one trajectory per agent");
    const long long n = (long long)sc->NA * T * VG;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(veh_coll_bwd_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       veh_args(sc, pair_off, P, traj, T, cent_x, rad, buffer), d_pen, amin, d_traj, VehImplicit{});
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// =============================================================================================
// interp_traj (reference src/losses/adv_gen_nusc.py:625-644): linear up-sampling in time of (x,y,hx,hy) by an
// integer factor (F.interpolate(mode='linear', align_corners=False)) followed by renormalisation of the heading.
// torch's generic upsample backward costs 1.9 ms per call here (atomics); this pair is a thread per output /
// per input element with the tap tables (i0, i1, w0, w1 per output step, computed on the host in fp32 exactly
// like ATen's area_pixel_compute_source_index) passed in.
// =============================================================================================
__global__ __launch_bounds__(256) void interp_traj_fwd_kernel(const float* __restrict__ in, int N, int T, int TO,
                                                                const int32_t* __restrict__ i0, const int32_t* __restrict__ i1,
                                                                const float* __restrict__ w0, const float* __restrict__ w1,
                                                                float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * TO) return;
    const int n = idx / TO, j = idx - n * TO;
    const float* a = in + ((size_t)n * T + i0[j]) * 4;
    const float* b = in + ((size_t)n * T + i1[j]) * 4;
    float u[4];
    for (int c = 0; c < 4; ++c) u[c] = __fadd_rn(__fmul_rn(w0[j], a[c]), __fmul_rn(w1[j], b[c]));
    const float nrm = sqrtf(u[2] * u[2] + u[3] * u[3]);
    float* o = out + (size_t)idx * 4;
    o[0] = u[0];
    o[1] = u[1];
    o[2] = u[2] / nrm;
    o[3] = u[3] / nrm;
}

// d_in[n][t] = sum over outputs j that tap t of  w * d_u[j],  d_u = adjoint of the pre-normalisation lerp
__global__ __launch_bounds__(256) void interp_traj_bwd_kernel(const float* __restrict__ in, const float* __restrict__ d_out,
                                                                int N, int T, int TO, int scale,
                                                                const int32_t* __restrict__ i0, const int32_t* __restrict__ i1,
                                                                const float* __restrict__ w0, const float* __restrict__ w1,
                                                                float* __restrict__ d_in) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * T) return;
    const int n = idx / T, t = idx - n * T;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    int jlo = (t - 1) * scale - scale, jhi = (t + 1) * scale + scale;
    jlo = jlo < 0 ? 0 : jlo;
    jhi = jhi > TO - 1 ? TO - 1 : jhi;
    for (int j = jlo; j <= jhi; ++j) {
        const int a0 = i0[j], a1 = i1[j];
        float w = 0.f;
        if (a0 == t) w += w0[j];
        if (a1 == t) w += w1[j];
        if (w == 0.f) continue;
        const float* a = in + ((size_t)n * T + a0) * 4;
        const float* b = in + ((size_t)n * T + a1) * 4;
        const float u2 = __fadd_rn(__fmul_rn(w0[j], a[2]), __fmul_rn(w1[j], b[2]));
        const float u3 = __fadd_rn(__fmul_rn(w0[j], a[3]), __fmul_rn(w1[j], b[3]));
        const float nrm = sqrtf(u2 * u2 + u3 * u3);
        const float o2 = u2 / nrm, o3 = u3 / nrm;
        const float* go = d_out + ((size_t)n * TO + j) * 4;
        const float dot = o2 * go[2] + o3 * go[3];
        g[0] += w * go[0];
        g[1] += w * go[1];
        g[2] += w * (go[2] - o2 * dot) / nrm;
        g[3] += w * (go[3] - o3 * dot) / nrm;
    }
    float* o = d_in + (size_t)idx * 4;
    for (int c = 0; c < 4; ++c) o[c] = g[c];
}

extern "C" int strive_interp_traj_fwd(const float* in, int32_t N, int32_t T, int32_t TO, const int32_t* i0, const int32_t* i1,
                                      const float* w0, const float* w1, float* out, strive_stream_t stream) {
    STRIVE_CHECK_ARG(in && i0 && i1 && w0 && w1 && out, "null argument");
    if (N <= 0 || TO <= 0) return 0;
    hipLaunchKernelGGL(interp_traj_fwd_kernel, dim3((N * TO + 255) / 256), dim3(256), 0, (hipStream_t)stream, in, N, T, TO, i0,
                       i1, w0, w1, out);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int strive_interp_traj_bwd(const float* in, const float* d_out, int32_t N, int32_t T, int32_t TO, int32_t scale,
                                      const int32_t* i0, const int32_t* i1, const float* w0, const float* w1, float* d_in,
                                      strive_stream_t stream) {
    STRIVE_CHECK_ARG(in && d_out && i0 && i1 && w0 && w1 && d_in, "null argument");
    STRIVE_CHECK_ARG(scale >= 1, "bad scale");
    if (N <= 0 || T <= 0) return 0;
    hipLaunchKernelGGL(interp_traj_bwd_kernel, dim3((N * T + 255) / 256), dim3(256), 0, (hipStream_t)stream, in, d_out, N, T, TO,
                       scale, i0, i1, w0, w1, d_in);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// =============================================================================================
// AvoidCollLoss (reference src/losses/adv_gen_nusc.py:264-341) and AdvGenLoss (:53-262) in one call per direction.
//   AvoidCollLoss forward : interp_traj_fwd -> veh_coll_fwd -> coll_point (rows) -> loss_partial<false> -> avoid_final  (5 launches)
//                 backward: loss_grad<false> (environment term, d_z) -> veh_coll_bwd<implicit> -> interp_traj_bwd            (3 launches)
//   AdvGenLoss    forward : interp -> veh_coll_fwd -> coll_point (non-ego rows) -> adv_crash (one workgroup per scene: distances to
//                           the target, behind test, per-scene soft-min, crash term, prior re-weights) -> loss_partial<true> ->
//                           adv_final                                                                                   (6 launches)
//                 backward: loss_grad<true> (environment term, d_z) -> veh_coll_bwd<implicit, per-slot weights> -> interp_bwd -> adv_crash_bwd
// against ~60 + ~45 (AvoidCollLoss) and ~140 + ~110 (AdvGenLoss) elementwise / scatter torch operators.  All sums are float64
// partials per workgroup added in a fixed order (deterministic); the means divide by max(count, 1) like the reference's "[0.]
// when nothing collides" sentinel does.  AdvGenLoss is AvoidCollLoss plus the planner pairs, the per-row re-weights and the
// crash term, and is written that way: AdvArgs / AdvWs embed AvoidArgs / AvoidWs, the partial-sum and gradient kernels are
// templates over the objective (the AvoidCollLoss forms compile none of AdvGenLoss's loads), and the
// two host sequences share their stages.
// The "every attacker is always behind its target" escape (:120-123) is a property of the whole batch: adv_crash evaluates the
// soft-min with and without the behind mask and leaves a per-scene flag; the kernels after it form the batch-wide AND themselves
// and pick the variant.
// =============================================================================================
extern "C" int strive_coll_point_rows(const StriveMap* map, const float* fine, int32_t TO, const int32_t* agent_of,
                                      const float* lw, const int32_t* mapix, int32_t NE, int32_t gl, int32_t gw,
                                      const float* lin_l, const float* lin_w, float* out_pt, int32_t* out_cnt,
                                      strive_stream_t stream);

#define AV_BLOCKS 1024
#define NT_AV 256
#define ADV_MAXE 1024       // (non-ego agents of a scene) x (crash time samples) the crash kernel keeps in LDS

// out[] of the two forward calls (ABI, include/strive_hip.h): the named slots, zeros from *_END up to *_SIZE
enum AvoidOut { AO_LOSS, AO_VEH, AO_ENV, AO_PRIOR, AO_INIT, AO_VEH_N, AO_ENV_N, AO_END, AO_SIZE = 8 };
enum AdvOut { DO_LOSS, DO_VEH, DO_PLAN, DO_ENV, DO_PRIOR, DO_INIT, DO_CRASH, DO_VEH_N, DO_PLAN_N, DO_ENV_N, DO_SEL, DO_END, DO_SIZE = 16 };

struct AvoidWs {
    float* fine;            // (NA,TO,4)
    float* pen;             // (TO,P)
    uint8_t* hit;           // (TO,P)
    uint8_t* amin;          // (TO,P)
    float* pt;              // (NE*TO,2)
    int32_t* cnt;           // (NE*TO)
    double* partial;        // (AV_BLOCKS, AV_TERMS)
    double* sums;           // (AV_TERMS)
    float* d_fine;          // (NA,TO,4) backward scratch
};

struct AdvWs {
    AvoidWs av;
    double* partial;        // (AV_BLOCKS, ADV_TERMS)
    double* sums;           // (ADV_SUMS)
    float* soft2;           // (2, NE, NT)   variant 0 = with the behind mask, 1 = without
    float* rew2;            // (2, NE)
    float* crash2;          // (2, B)
    int32_t* scene_flag;    // (B) 1 = every non-ego agent of the scene is always behind
    int32_t* sel;           // (1) chosen variant
    float* rew_sel;         // (NE) re-weights of the chosen variant (the backward kernels read these)
};

// Each workspace is laid out by ONE function, which carves it from the caller's buffer and -- over a null base of unlimited
// capacity, where the arena's offset is the size -- measures it; both end in 256 bytes of slack.
static AvoidWs avoid_layout(StriveArena& ar, size_t NA, size_t TO, size_t P, size_t NE) {
    AvoidWs w;
    w.fine = ar.take<float>(NA * TO * 4);
    w.d_fine = ar.take<float>(NA * TO * 4);
    w.pen = ar.take<float>(TO * P);
    w.hit = ar.take<uint8_t>(TO * P);
    w.amin = ar.take<uint8_t>(TO * P);
    w.pt = ar.take<float>(NE * TO * 2);
    w.cnt = ar.take<int32_t>(NE * TO);
    w.partial = ar.take<double>((size_t)AV_BLOCKS * AV_TERMS);
    w.sums = ar.take<double>(AV_TERMS);
    ar.take<char>(256);
    return w;
}

static AdvWs adv_layout(StriveArena& ar, size_t NA, size_t TO, size_t P, size_t NE, size_t NT, size_t B) {
    AdvWs w;
    w.av = avoid_layout(ar, NA, TO, P, NE);
    w.partial = ar.take<double>((size_t)AV_BLOCKS * ADV_TERMS);
    w.sums = ar.take<double>(ADV_SUMS);
    w.soft2 = ar.take<float>(2 * NE * NT);
    w.rew2 = ar.take<float>(2 * NE);
    w.crash2 = ar.take<float>(2 * B);
    w.scene_flag = ar.take<int32_t>(B);
    w.sel = ar.take<int32_t>(1);
    w.rew_sel = ar.take<float>(NE);
    ar.take<char>(256);
    return w;
}

static size_t avoid_ws_bytes(size_t NA, size_t TO, size_t P, size_t NE) {
    StriveArena ar(nullptr, SIZE_MAX);
    avoid_layout(ar, NA, TO, P, NE);
    return ar.off;
}

static size_t adv_ws_bytes(size_t NA, size_t TO, size_t P, size_t NE, size_t NT, size_t B) {
    StriveArena ar(nullptr, SIZE_MAX);
    adv_layout(ar, NA, TO, P, NE, NT, B);
    return ar.off;
}

struct AvoidArgs {
    int NA, TO, P, NE, NZ, D;
    float prior_den, init_den;
    const float* fine;
    const float* pen;
    const uint8_t* hit;
    const uint8_t* valid;
    const int32_t* env_agent;
    const float* pt;
    const float* pdist;
    const float *z, *mu, *var, *init_z;
    float w_veh, w_env, w_prior, w_init;
    const uint8_t* scene_alive;     // (B) or null; AdvGenLoss only (a quarantined scene's rows count as "no collision point")
    const int32_t* scene_of;        // (NA)
};

struct AdvArgs {
    AvoidArgs a;
    int B, T, t0, NT, use_infront;
    float infront;
    const float* traj;          // (NA,T,4)
    const float* tgt;           // (B,T,4)
    const int32_t* ne_ptr;
    const int32_t* nonego;      // (NE) agent index
    const int32_t* slot_ne;
    const uint8_t* atk_mask;
    const uint8_t* scene_alive;     // (B) or null
    float w_crash, w_plan, w_prior_atk, w_init_atk;
    float* soft2;
    float* rew2;
    float* crash2;
    int32_t* scene_flag;
    float* rew_sel;
};

// what a kernel written for both objectives takes, and the AvoidCollLoss part of it
template <bool ADV> using LossArgs = typename std::conditional<ADV, AdvArgs, AvoidArgs>::type;
__device__ __forceinline__ const AvoidArgs& avoid_part(const AvoidArgs& a) { return a; }
__device__ __forceinline__ const AvoidArgs& avoid_part(const AdvArgs& A) { return A.a; }

// off-road penalty of row (e, t): 1 - |c - p| / r for rows with a collision point (reference :384-403)
__device__ __forceinline__ bool env_row(const AvoidArgs& a, int row, float& dx, float& dy, float& d, float& pd) {
    const float px = a.pt[(size_t)row * 2], py = a.pt[(size_t)row * 2 + 1];
    if (!(px + py == px + py)) return false;      // NaN point = no collision point
    const int e = row / a.TO, t = row - e * a.TO;
    if (a.scene_alive && !a.scene_alive[a.scene_of[a.env_agent[e]]]) return false;
    const float* c = a.fine + ((size_t)a.env_agent[e] * a.TO + t) * 4;
    dx = c[0] - px;
    dy = c[1] - py;
    d = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
    pd = a.pdist[e];
    return true;
}

// -log N(z; mu, var) per element as losses/common.py:26-41 evaluates it in fp32
__device__ __forceinline__ float prior_nll(float z, float mu, float var) {
    const float dz = z - mu;
    return -(-logf(sqrtf(var)) - 0.91893853320467267f - (dz * dz) / (2.0f * var));
}
__device__ __forceinline__ float init_sq(float z, float init) {
    const float di = init - z;
    return di * di;
}
// AdvGenLoss: weight of a latent row's prior / init term, blended by its re-weight (reference :160-167, :227-231)
__device__ __forceinline__ float atk_blend(float rw, float w, float w_atk) { return rw * w + (1.0f - rw) * w_atk; }
__device__ __forceinline__ bool latent_row_alive(const AdvArgs& A, int r) {
    return !(A.scene_alive && !A.scene_alive[A.a.scene_of[A.nonego[r]]]);
}
__device__ __forceinline__ double masked_mean(double sum, double count) { return sum / (count < 1.0 ? 1.0 : count); }

// block-wide reductions of a 256-thread workgroup in a fixed order (wave tree, then the four waves pairwise)
__device__ __forceinline__ double sum_waves_d(const double* w) { return (w[0] + w[1]) + (w[2] + w[3]); }
__device__ __forceinline__ double block_sum_d(double v, double* s_red, int tid) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = v;
    __syncthreads();
    return sum_waves_d(s_red);
}
__device__ __forceinline__ float block_max_f(float v, float* s_red, int tid) {
    v = wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

// batch-wide "everybody is always behind" test -> variant 1 (no behind mask); every workgroup that needs it forms it itself
__device__ __forceinline__ int adv_select(const int32_t* scene_flag, int B, int use_infront, int tid) {
    __shared__ int s_all;
    if (tid == 0) s_all = use_infront ? 1 : 0;
    __syncthreads();
    int all = 1;
    for (int b = tid; b < B; b += blockDim.x) all &= scene_flag[b];
    if (!all) s_all = 0;                 // (every writer stores the same value)
    __syncthreads();
    return s_all;
}

// Per-workgroup partial sums of the LossSum terms of either objective.  AdvGenLoss (ADV) picks the soft-min variant first, sends
// the planner-involving slots (slot_ne >= 0) to their own re-weighted accumulator, blends the weight of every latent row by
// its re-weight and skips the rows of quarantined scenes; the AvoidCollLoss form compiles none of that.
template <bool ADV>
__global__ __launch_bounds__(256) void loss_partial_kernel(LossArgs<ADV> A, double* __restrict__ partial) {
    constexpr int NTERMS = ADV ? ADV_TERMS : AV_TERMS;
    __shared__ double s_red[NTERMS][4];
    const AvoidArgs& a = avoid_part(A);
    const int tid = threadIdx.x;
    const float* rew = nullptr;
    float w_plan = 0.f;
    if constexpr (ADV) {
        rew = A.rew2 + (size_t)adv_select(A.scene_flag, A.B, A.use_infront, tid) * a.NE;
        w_plan = A.w_plan;
    }
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long g0 = (long long)blockIdx.x * blockDim.x + tid;
    double acc[NTERMS] = {};
    if (a.w_veh > 0.f || w_plan > 0.f) {
        // (t, slot) walked with 32-bit indices: slot fastest, so pen / hit reads are contiguous and `valid` stays in L1
        const int per_t = (a.P + NT_AV - 1) / NT_AV;                 // slot chunks of one time sample
        const long long nchunk = (long long)a.TO * per_t;
        for (long long ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
            const int t = (int)(ch / per_t), slot = (int)(ch - (long long)t * per_t) * NT_AV + tid;
            if (slot < a.P) {
                const size_t i = (size_t)t * a.P + slot;
                if (a.hit[i] && a.valid[slot]) {          // (pen is only valid behind hit)
                    bool planner = false;
                    if constexpr (ADV) {
                        const int ne = A.slot_ne[slot];
                        planner = ne >= 0;
                        if (planner && w_plan > 0.f) { acc[S_PLAN] += (double)(a.pen[i] * rew[ne]); acc[S_PLAN_N] += 1.0; }
                    }
                    if (!planner && a.w_veh > 0.f) { acc[S_VEH] += (double)a.pen[i]; acc[S_VEH_N] += 1.0; }
                }
            }
        }
    }
    if (a.w_env > 0.f) {
        const long long n = (long long)a.NE * a.TO;
        for (long long i = g0; i < n; i += stride) {
            float dx, dy, d, pd;
            if (env_row(a, (int)i, dx, dy, d, pd)) { acc[S_ENV] += (double)(1.0f - d / pd); acc[S_ENV_N] += 1.0; }
        }
    }
    if (a.w_prior > 0.f || a.w_init > 0.f) {
        const long long n = (long long)a.NZ * a.D;
        for (long long i = g0; i < n; i += stride) {
            float rw = 0.f;
            if constexpr (ADV) {
                const int r = (int)(i / a.D);
                if (!latent_row_alive(A, r)) continue;
                rw = rew[r];
            }
            const float z = a.z[i];
            if (a.w_prior > 0.f) {
                const float nll = prior_nll(z, a.mu[i], a.var[i]);
                if constexpr (ADV) acc[S_PRIOR] += (double)(nll * atk_blend(rw, a.w_prior, A.w_prior_atk));
                else acc[S_PRIOR] += (double)nll;
            }
            if (a.w_init > 0.f) {
                const float sq = init_sq(z, a.init_z[i]);
                if constexpr (ADV) acc[S_INIT] += (double)(sq * atk_blend(rw, a.w_init, A.w_init_atk));
                else acc[S_INIT] += (double)sq;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NTERMS; ++k) acc[k] = wave_sum_d(acc[k]);
    if ((tid & 63) == 0)
        for (int k = 0; k < NTERMS; ++k) s_red[k][tid >> 6] = acc[k];
    __syncthreads();
    if (tid < NTERMS) partial[(size_t)blockIdx.x * NTERMS + tid] = sum_waves_d(s_red[tid]);
}

// s[k] = sums[k] = term k added over the workgroup partials, one wave: lanes stride over the partials, then a shuffle tree -- a
// fixed order (deterministic), 16 steps instead of 1024
template <int NTERMS>
__device__ __forceinline__ void sum_partials(const double* __restrict__ partial, int nblocks, int tid, double* s, double* sums) {
    for (int k = 0; k < NTERMS; ++k) {
        double v = 0.0;
        for (int b = tid; b < nblocks; b += 64) v += partial[(size_t)b * NTERMS + k];
        v = wave_sum_d(v);
        if (tid == 0) { s[k] = v; sums[k] = v; }
    }
}

__global__ __launch_bounds__(64) void avoid_final_kernel(AvoidArgs a, const double* __restrict__ partial, int nblocks,
                                                           double* __restrict__ sums, float* __restrict__ out) {
    __shared__ double s[AV_TERMS];
    const int tid = threadIdx.x;
    sum_partials<AV_TERMS>(partial, nblocks, tid, s, sums);
    __syncthreads();
    if (tid == 0) {
        const double veh = masked_mean(s[S_VEH], s[S_VEH_N]);
        const double env = masked_mean(s[S_ENV], s[S_ENV_N]);
        const double pri = a.prior_den > 0.f ? s[S_PRIOR] / (double)a.prior_den : 0.0;
        const double ini = a.init_den > 0.f ? s[S_INIT] / (double)a.init_den : 0.0;
        double loss = 0.0;
        if (a.w_veh > 0.f) loss += (double)a.w_veh * veh;
        if (a.w_env > 0.f) loss += (double)a.w_env * env;
        if (a.w_prior > 0.f) loss += (double)a.w_prior * pri;
        if (a.w_init > 0.f) loss += (double)a.w_init * ini;
        out[AO_LOSS] = (float)loss;
        out[AO_VEH] = (float)veh;
        out[AO_ENV] = (float)env;
        out[AO_PRIOR] = (float)pri;
        out[AO_INIT] = (float)ini;
        out[AO_VEH_N] = (float)s[S_VEH_N];
        out[AO_ENV_N] = (float)s[S_ENV_N];
        for (int k = AO_END; k < AO_SIZE; ++k) out[k] = 0.f;
    }
}

__global__ __launch_bounds__(64) void adv_final_kernel(AdvArgs A, const double* __restrict__ partial, int nblocks,
                                                         double* __restrict__ sums, int32_t* __restrict__ sel_out,
                                                         float* __restrict__ out, float* __restrict__ soft,
                                                         float* __restrict__ rew) {
    __shared__ double s[ADV_LOCAL];
    const AvoidArgs& a = A.a;
    const int tid = threadIdx.x;
    const int sel = adv_select(A.scene_flag, A.B, A.use_infront, tid);
    sum_partials<ADV_TERMS>(partial, nblocks, tid, s, sums);
    {
        double v = 0.0, rows = 0.0, scenes = 0.0;
        for (int b = tid; b < A.B; b += 64) {
            v += (double)A.crash2[(size_t)sel * A.B + b];
            if (!A.scene_alive || A.scene_alive[b]) { scenes += 1.0; rows += (double)(A.ne_ptr[b + 1] - A.ne_ptr[b]); }
        }
        v = wave_sum_d(v);
        rows = wave_sum_d(rows);
        scenes = wave_sum_d(scenes);
        if (tid == 0) { s[S_CRASH] = v; s[S_ROWS] = sums[S_ROWS] = rows; s[S_SCENES] = sums[S_SCENES] = scenes; }
    }
    // the selected soft-min weights and re-weights, for the caller (return_mins, logging)
    for (long long i = tid; i < (long long)a.NE * A.NT; i += 64) soft[i] = A.soft2[(size_t)sel * a.NE * A.NT + i];
    for (int i = tid; i < a.NE; i += 64) {
        const float rv = A.rew2[(size_t)sel * a.NE + i];
        rew[i] = rv;
        A.rew_sel[i] = rv;
    }
    __syncthreads();
    if (tid == 0) {
        const double veh = masked_mean(s[S_VEH], s[S_VEH_N]);
        const double env = masked_mean(s[S_ENV], s[S_ENV_N]);
        const double plan = masked_mean(s[S_PLAN], s[S_PLAN_N]);
        // means over the latent rows / scenes that are in the batch: all of them, or the alive ones (= the batch rebuilt
        // without the quarantined scenes, which is what the reference's batch_size-1 runs amount to)
        const double pri = s[S_ROWS] > 0.0 ? s[S_PRIOR] / s[S_ROWS] : 0.0;
        const double ini = s[S_INIT];
        const double crash = s[S_SCENES] > 0.0 ? s[S_CRASH] / s[S_SCENES] : 0.0;
        double loss = 0.0;
        if (a.w_init > 0.f) loss += ini;
        if (a.w_prior > 0.f) loss += pri;
        if (a.w_veh > 0.f) loss += (double)a.w_veh * veh;
        if (A.w_plan > 0.f) loss += (double)A.w_plan * plan;
        if (a.w_env > 0.f) loss += (double)a.w_env * env;
        if (A.w_crash > 0.f) loss += (double)A.w_crash * crash;
        sel_out[0] = sel;
        out[DO_LOSS] = (float)loss;
        out[DO_VEH] = (float)veh;
        out[DO_PLAN] = (float)plan;
        out[DO_ENV] = (float)env;
        out[DO_PRIOR] = (float)pri;
        out[DO_INIT] = (float)ini;
        out[DO_CRASH] = (float)crash;
        out[DO_VEH_N] = (float)s[S_VEH_N];
        out[DO_PLAN_N] = (float)s[S_PLAN_N];
        out[DO_ENV_N] = (float)s[S_ENV_N];
        out[DO_SEL] = (float)sel;
        for (int k = DO_END; k < DO_SIZE; ++k) out[k] = 0.f;
    }
}

// The (NA, TO) rows of d_fine, then the (NZ, D) elements of d_z.  d_fine gets the environment term -- every row is written, zeros
// where the agent takes no environment term or has no collision point, so the vehicle term can accumulate on top without a
// memset; only the latent half differs between the objectives.
template <bool ADV>
__global__ __launch_bounds__(256) void loss_grad_kernel(LossArgs<ADV> A, const int32_t* __restrict__ env_of_agent,
                                                          const double* __restrict__ sums, const float* __restrict__ d_loss,
                                                          float* __restrict__ d_fine, float* __restrict__ d_z) {
    const AvoidArgs& a = avoid_part(A);
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n_rows = (long long)a.NA * a.TO;
    const float gl = d_loss[0];
    if (idx < n_rows) {
        const int ag = (int)(idx / a.TO), t = (int)(idx - (long long)ag * a.TO);
        float gx = 0.f, gy = 0.f;
        const int e = (a.w_env > 0.f && env_of_agent) ? env_of_agent[ag] : -1;
        if (e >= 0) {
            float dx, dy, d, pd;
            if (env_row(a, e * a.TO + t, dx, dy, d, pd) && d > 0.f) {
                const float gs = (float)masked_mean((double)gl * (double)a.w_env, sums[S_ENV_N]);
                const float k = -gs / (d * pd);      // pen = 1 - d / pd  ->  d pen / d c = -(c - p) / (d * pd)
                gx = k * dx;
                gy = k * dy;
            }
        }
        float* o = d_fine + (size_t)idx * 4;
        o[0] = gx; o[1] = gy; o[2] = 0.f; o[3] = 0.f;
        return;
    }
    const long long i = idx - n_rows;
    if (i < (long long)a.NZ * a.D) {
        const float z = a.z[i];
        float g = 0.f;
        if constexpr (ADV) {
            const int r = (int)(i / a.D);
            const float rw = A.rew_sel[r];
            if (latent_row_alive(A, r)) {
                if (a.w_prior > 0.f) g += gl * atk_blend(rw, a.w_prior, A.w_prior_atk) / (float)sums[S_ROWS] * ((z - a.mu[i]) / a.var[i]);
                if (a.w_init > 0.f) g += gl * atk_blend(rw, a.w_init, A.w_init_atk) * (2.0f * (z - a.init_z[i]));
            }
        } else {
            if (a.w_prior > 0.f) g += gl * a.w_prior / a.prior_den * ((z - a.mu[i]) / a.var[i]);
            if (a.w_init > 0.f) g += gl * a.w_init / a.init_den * (2.0f * (z - a.init_z[i]));
        }
        d_z[i] = g;
    }
}

// entry e = (non-ego agent, crash time sample) of scene b, whose non-ego rows start at a0: attacker position minus target position
// and its length; returns the offset of the attacker's pose in traj / d_traj and leaves the target's pose in q
__device__ __forceinline__ size_t crash_entry(const AdvArgs& A, int b, int a0, int e, const float*& q, float& dx, float& dy, float& d) {
    const int al = e / A.NT, t = e - al * A.NT;
    const size_t at = ((size_t)A.nonego[a0 + al] * A.T + A.t0 + t) * 4;
    q = A.tgt + ((size_t)b * A.T + A.t0 + t) * 4;
    dx = A.traj[at] - q[0];
    dy = A.traj[at + 1] - q[1];
    d = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
    return at;
}

// one workgroup per scene
__global__ __launch_bounds__(256) void adv_crash_kernel(AdvArgs A) {
    __shared__ float s_d[ADV_MAXE];
    __shared__ float s_s[ADV_MAXE];
    __shared__ int s_nb[64];             // per non-ego agent: time samples at which it is NOT behind the target
    __shared__ double s_redd[4];
    __shared__ float s_redf[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int a0 = A.ne_ptr[b], n = A.ne_ptr[b + 1] - a0, NT = A.NT, E = n * NT;
    if (A.scene_alive && !A.scene_alive[b]) {
        // quarantined scene (its planner failed, StriveAdvGen.scene_alive): no crash term, no soft-min weights, re-weights 1, and
        // like an empty scene it does not veto the batch-wide "everybody is behind" test
        for (int v = 0; v < 2; ++v) {
            for (int e = tid; e < E; e += 256) A.soft2[((size_t)v * A.a.NE + a0) * NT + e] = 0.f;
            for (int al = tid; al < n; al += 256) A.rew2[(size_t)v * A.a.NE + a0 + al] = 1.0f;
            if (tid == 0) A.crash2[(size_t)v * A.B + b] = 0.f;
        }
        if (tid == 0) A.scene_flag[b] = 1;
        return;
    }
    if (tid < 64) s_nb[tid] = 0;
    __syncthreads();
    for (int e = tid; e < E; e += 256) {
        const float* q;
        float dx, dy, d;
        crash_entry(A, b, a0, e, q, dx, dy, d);
        s_d[e] = d;
        if (A.use_infront) {
            // behind <=> (atk - tgt) / |atk - tgt| . heading(tgt) < threshold   (reference :646-673); NaN compares false
            const float dot = __fadd_rn(__fmul_rn(dx / d, q[2]), __fmul_rn(dy / d, q[3]));
            if (!(dot < A.infront)) atomicAdd(&s_nb[e / NT], 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int all_always = A.use_infront ? 1 : 0;
        for (int al = 0; al < n; ++al) all_always &= (s_nb[al] == 0);
        A.scene_flag[b] = all_always;            // (an empty scene leaves 1: it does not veto the batch-wide test)
    }
    for (int v = 0; v < 2; ++v) {
        // entry e is out of the soft-min: its agent is always behind (variant 0 only) or not among the selected attackers
        auto masked = [&](int e) {
            const int al = e / NT;
            return (v == 0 && A.use_infront && s_nb[al] == 0) || (A.atk_mask && !A.atk_mask[a0 + al]);
        };
        float mx = -3.0e38f;
        for (int e = tid; e < E; e += 256) {
            const float d = s_d[e];
            if (!masked(e) && !(d != d)) mx = fmaxf(mx, -d);
        }
        mx = block_max_f(mx, s_redf, tid);
        double den = 0.0;
        for (int e = tid; e < E; e += 256) {
            const float ex = masked(e) ? 0.f : expf(-s_d[e] - mx);
            s_s[e] = ex;
            den += (double)ex;
        }
        den = block_sum_d(den, s_redd, tid);
        const bool dead = !(den > 0.0) || mx <= -3.0e38f;          // nothing unmasked (or NaN distances): all weights 0 (:134-135)
        double cr = 0.0;
        for (int e = tid; e < E; e += 256) {
            const float sft = dead ? 0.f : (float)((double)s_s[e] / den);
            s_s[e] = sft;
            const float d = s_d[e];
            cr += (double)(sft * (d * d));
            A.soft2[((size_t)v * A.a.NE + a0) * NT + e] = sft;
        }
        cr = block_sum_d(cr, s_redd, tid);
        if (tid == 0) A.crash2[(size_t)v * A.B + b] = (float)cr;
        for (int al = tid; al < n; al += 256) {
            float sm = 0.f;
            for (int t = 0; t < NT; ++t) sm += s_s[al * NT + t];
            A.rew2[(size_t)v * A.a.NE + a0 + al] = 1.0f - sm;
        }
        __syncthreads();
    }
}

// crash term: L = w/B sum_b sum_e s_e d_e^2 with s = softmin(d) over the scene's unmasked entries
//   dL/dd_e = w/B * s_e * (2 d_e + C_b - d_e^2),  C_b = sum_e s_e d_e^2;   dd/d(atk xy) = (atk - tgt) / d = -dd/d(tgt xy)
// one workgroup per scene: adds into d_traj (non-ego rows, time >= t0; interp_bwd has written them) and writes d_tgt
__global__ __launch_bounds__(256) void adv_crash_bwd_kernel(AdvArgs A, const int32_t* __restrict__ sel_p, const double* __restrict__ sums,
                                                              const float* __restrict__ d_loss, float* __restrict__ d_traj,
                                                              float* __restrict__ d_tgt) {
    __shared__ float s_gx[ADV_MAXE], s_gy[ADV_MAXE];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int sel = sel_p[0];
    const int a0 = A.ne_ptr[b], n = A.ne_ptr[b + 1] - a0, NT = A.NT, E = n * NT;
    const float C = A.crash2[(size_t)sel * A.B + b];
    const float gw = A.w_crash > 0.f ? d_loss[0] * A.w_crash / (float)sums[S_SCENES] : 0.f;      // (a quarantined scene has soft == 0 throughout)
    for (int e = tid; e < E; e += 256) {
        const float* q;
        float dx, dy, d;
        float* gp = d_traj + crash_entry(A, b, a0, e, q, dx, dy, d);
        const float sft = A.soft2[((size_t)sel * A.a.NE + a0) * NT + e];
        float gx = 0.f, gy = 0.f;
        if (sft != 0.f && d > 0.f) {
            const float gd = gw * sft * (2.0f * d + C - d * d);
            gx = gd * dx / d;
            gy = gd * dy / d;
        }
        gp[0] += gx;
        gp[1] += gy;
        s_gx[e] = gx;
        s_gy[e] = gy;
    }
    __syncthreads();
    for (int t = tid; t < A.T; t += 256) {
        float sx = 0.f, sy = 0.f;
        if (t >= A.t0)
            for (int al = 0; al < n; ++al) { sx += s_gx[al * NT + t - A.t0]; sy += s_gy[al * NT + t - A.t0]; }
        float* o = d_tgt + ((size_t)b * A.T + t) * 4;
        o[0] = -sx; o[1] = -sy; o[2] = 0.f; o[3] = 0.f;
    }
}

static AvoidArgs avoid_args(const StriveScenes* sc, const StriveAvoidColl* h, const AvoidWs& w, int TO, const float* z,
                            const float* mu, const float* var) {
    AvoidArgs a;
    a.NA = sc->NA; a.TO = TO; a.P = h->P; a.NE = h->NE; a.NZ = h->NZ; a.D = h->D;
    a.prior_den = h->prior_den; a.init_den = h->init_den;
    a.fine = w.fine; a.pen = w.pen; a.hit = w.hit; a.valid = h->pair_valid;
    a.env_agent = h->env_agent; a.pt = w.pt; a.pdist = h->env_pdist;
    a.z = z; a.mu = mu; a.var = var; a.init_z = h->init_z;
    a.w_veh = h->w_veh; a.w_env = h->w_env; a.w_prior = h->w_prior; a.w_init = h->w_init;
    a.scene_alive = nullptr; a.scene_of = sc->scene_of;
    return a;
}

static AdvArgs adv_args(const StriveScenes* sc, const StriveAdvGen* h, const AdvWs& w, int T, const float* traj, const float* tgt,
                        const float* z, const float* mu, const float* var) {
    AdvArgs A;
    A.a = avoid_args(sc, &h->base, w.av, T * h->base.scale, z, mu, var);
    A.B = sc->B; A.T = T; A.t0 = h->t0; A.NT = T - h->t0; A.use_infront = h->use_infront; A.infront = h->infront;
    A.traj = traj; A.tgt = tgt; A.ne_ptr = h->ne_ptr; A.nonego = h->base.env_agent; A.slot_ne = h->slot_ne; A.atk_mask = h->atk_mask;
    A.scene_alive = h->scene_alive; A.a.scene_alive = h->scene_alive;
    A.w_crash = h->w_crash; A.w_plan = h->w_plan; A.w_prior_atk = h->w_prior_atk; A.w_init_atk = h->w_init_atk;
    A.soft2 = w.soft2; A.rew2 = w.rew2; A.crash2 = w.crash2; A.scene_flag = w.scene_flag; A.rew_sel = w.rew_sel;
    return A;
}

static int avoid_check(const StriveScenes* sc, const StriveAvoidColl* h, int T) {
    STRIVE_CHECK_ARG(sc && h, "null argument");
    STRIVE_CHECK_ARG(sc->NS == 1, "collision losses take one trajectory per agent");
    STRIVE_CHECK_ARG(T > 0 && h->scale >= 1 && h->P >= 0 && h->NE >= 0 && h->NZ >= 0 && h->D >= 0, "bad sizes");
    STRIVE_CHECK_ARG(h->i0 && h->i1 && h->w0 && h->w1, "null interpolation taps");
    if (h->w_veh > 0.f) STRIVE_CHECK_ARG(h->pair_off && h->cent_x && h->rad && h->pair_valid, "null vehicle-term constants");
    if (h->w_env > 0.f && h->NE > 0)
        STRIVE_CHECK_ARG(h->env_agent && h->env_of_agent && h->env_lw && h->env_mapix && h->env_pdist && h->lin_l && h->lin_w &&
                             h->gl > 0 && h->gw > 0,
                         "null environment-term constants");
    if (h->w_init > 0.f) STRIVE_CHECK_ARG(h->init_z, "null init_z");
    return 0;
}

static int adv_check(const StriveScenes* sc, const StriveAdvGen* h, int T) {
    STRIVE_CHECK_ARG(sc && h, "null argument");
    if (int rc = avoid_check(sc, &h->base, T)) return rc;
    STRIVE_CHECK_ARG(h->ne_ptr && h->slot_ne && h->base.env_agent && h->base.env_of_agent, "null scene tables");
    if (h->w_plan > 0.f) STRIVE_CHECK_ARG(h->base.pair_off && h->base.cent_x && h->base.rad && h->base.pair_valid, "null vehicle-term constants");
    STRIVE_CHECK_ARG(h->base.NE == sc->NA - sc->B && h->base.NZ == h->base.NE, "one latent row per non-ego agent");
    STRIVE_CHECK_ARG(h->t0 >= 0 && h->t0 < T, "bad crash_loss_min_time");
    STRIVE_CHECK_ARG(h->w_crash > 0.f, "the fused AdvGenLoss needs the crash term (its soft-min defines the re-weights)");
    STRIVE_CHECK_ARG(sc->max_n >= 1 && (sc->max_n - 1) * (T - h->t0) <= ADV_MAXE && sc->max_n - 1 <= 64,
                     "scene too large for the crash kernel's LDS tables");
    return 0;
}

// The stages both forwards open with: interp -> vehicle penalties (`veh`; far pairs culled on request, the pairs of scenes that
// are not `alive` written as not colliding) -> collision points
static int coll_forward_stages(const StriveScenes* sc, const StriveMap* map, const StriveAvoidColl* h, const float* traj, int T,
                               const AvoidWs& w, bool veh, int cull, const uint8_t* alive, strive_stream_t stream) {
    const int NA = sc->NA, TO = T * h->scale;
    if (NA <= 0) return 0;
    if (int rc = strive_interp_traj_fwd(traj, NA, T, TO, h->i0, h->i1, h->w0, h->w1, w.fine, stream)) return rc;
    if (veh)
        if (int rc = veh_coll_fwd_masked(sc, h->pair_off, h->P, w.fine, TO, h->cent_x, h->rad, h->buffer, alive, w.pen, w.hit, w.amin,
                                         stream, cull))
            return rc;
    if (h->w_env > 0.f && h->NE > 0)
        if (int rc = strive_coll_point_rows(map, w.fine, TO, h->env_agent, h->env_lw, h->env_mapix, h->NE, h->gl, h->gw, h->lin_l,
                                            h->lin_w, w.pt, w.cnt, stream))
            return rc;
    return 0;
}

// workgroups of the partial-sum kernel: 2048 elements of the longest of its three walks each
static int reduce_blocks(const StriveAvoidColl* h, int TO) {
    long long work = (long long)TO * h->P;
    if ((long long)h->NE * TO > work) work = (long long)h->NE * TO;
    if ((long long)h->NZ * h->D > work) work = (long long)h->NZ * h->D;
    const int nb = (int)((work + 2047) / 2048);
    return nb < 1 ? 1 : (nb > AV_BLOCKS ? AV_BLOCKS : nb);
}

// The stages both backwards share once d_fine holds the environment term: the vehicle term's implicit gradient on top (`veh`;
// AdvGenLoss passes slot_ne / rew_sel / w_plan for the planner pairs' second mean), then interp backward into d_traj
static int coll_backward_stages(const StriveScenes* sc, const StriveAvoidColl* h, const AvoidWs& w, const double* sums,
                                const float* traj, int T, const float* d_loss, float* d_traj, strive_stream_t stream, bool veh,
                                const int32_t* slot_ne = nullptr, const float* rew_sel = nullptr, float w_plan = 0.f) {
    const int NA = sc->NA, TO = T * h->scale;
    if (veh) {
        VehImplicit im;
        im.hit = w.hit; im.valid = h->pair_valid; im.sums = sums; im.d_loss = d_loss; im.w = h->w_veh;
        im.slot_ne = slot_ne; im.rew = rew_sel; im.w2 = w_plan;
        const long long nv = (long long)NA * TO * VG;
        hipLaunchKernelGGL(veh_coll_bwd_kernel<true>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           veh_args(sc, h->pair_off, h->P, w.fine, TO, h->cent_x, h->rad, h->buffer), (const float*)nullptr,
                           (const uint8_t*)w.amin, w.d_fine, im);
        STRIVE_CHECK_LAUNCH();
    }
    return strive_interp_traj_bwd(traj, w.d_fine, NA, T, TO, h->scale, h->i0, h->i1, h->w0, h->w1, d_traj, stream);
}

extern "C" size_t strive_avoid_coll_workspace_bytes(const StriveScenes* sc, const StriveAvoidColl* h, int32_t T) {
    if (!sc || !h || T <= 0 || h->scale < 1) return 0;
    return avoid_ws_bytes((size_t)sc->NA, (size_t)T * h->scale, (size_t)h->P, (size_t)h->NE);
}

extern "C" int strive_avoid_coll_fwd(const StriveScenes* sc, const StriveMap* map, const StriveAvoidColl* h, const float* traj,
                                     int32_t T, const float* z, const float* mu, const float* var, float* out, void* ws,
                                     size_t ws_bytes, strive_stream_t stream) {
    if (int rc = avoid_check(sc, h, T)) return rc;
    STRIVE_CHECK_ARG(traj && out && ws, "null argument");
    if (h->w_prior > 0.f) STRIVE_CHECK_ARG(z && mu && var, "null latent tensors");
    if (h->w_init > 0.f) STRIVE_CHECK_ARG(z, "null latent tensors");
    if (h->w_env > 0.f && h->NE > 0) STRIVE_CHECK_ARG(map, "null map");
    const int NA = sc->NA, TO = T * h->scale;
    STRIVE_CHECK_ARG(ws_bytes >= avoid_ws_bytes(NA, TO, h->P, h->NE), "workspace too small");
    StriveArena ar(ws, ws_bytes);
    const AvoidWs w = avoid_layout(ar, NA, TO, h->P, h->NE);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = coll_forward_stages(sc, map, h, traj, T, w, h->w_veh > 0.f && h->P > 0, /*cull=*/1, nullptr, stream)) return rc;
    AvoidArgs a = avoid_args(sc, h, w, TO, z, mu, var);
    if (h->P == 0) a.w_veh = 0.f;          // nothing to sum; the weight is re-applied below (mean of nothing = 0)
    if (h->NE == 0) a.w_env = 0.f;
    const int nb = reduce_blocks(h, TO);
    hipLaunchKernelGGL(loss_partial_kernel<false>, dim3(nb), dim3(256), 0, st, a, w.partial);
    STRIVE_CHECK_LAUNCH();
    hipLaunchKernelGGL(avoid_final_kernel, dim3(1), dim3(64), 0, st, a, (const double*)w.partial, nb, w.sums, out);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int strive_avoid_coll_bwd(const StriveScenes* sc, const StriveAvoidColl* h, const float* traj, int32_t T,
                                     const float* z, const float* mu, const float* var, const float* d_loss, void* ws,
                                     size_t ws_bytes, float* d_traj, float* d_z, strive_stream_t stream) {
    if (int rc = avoid_check(sc, h, T)) return rc;
    STRIVE_CHECK_ARG(traj && d_loss && ws && d_traj, "null argument");
    const int NA = sc->NA, TO = T * h->scale;
    STRIVE_CHECK_ARG(ws_bytes >= avoid_ws_bytes(NA, TO, h->P, h->NE), "workspace too small");
    if (NA == 0) return 0;
    StriveArena ar(ws, ws_bytes);
    const AvoidWs w = avoid_layout(ar, NA, TO, h->P, h->NE);
    AvoidArgs a = avoid_args(sc, h, w, TO, z, mu, var);
    if (h->NE == 0) a.w_env = 0.f;
    const bool latent = (h->w_prior > 0.f || h->w_init > 0.f) && h->D > 0;
    if (latent) STRIVE_CHECK_ARG(z && d_z && (h->w_prior <= 0.f || (mu && var)), "null latent tensors");
    if (!latent) a.D = 0;
    const long long n = (long long)NA * TO + (long long)a.NZ * a.D;
    hipLaunchKernelGGL(loss_grad_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, h->env_of_agent,
                       (const double*)w.sums, d_loss, w.d_fine, d_z);
    STRIVE_CHECK_LAUNCH();
    return coll_backward_stages(sc, h, w, w.sums, traj, T, d_loss, d_traj, stream, h->w_veh > 0.f && h->P > 0);
}

extern "C" size_t strive_adv_gen_workspace_bytes(const StriveScenes* sc, const StriveAdvGen* h, int32_t T) {
    if (!sc || !h || T <= 0 || h->base.scale < 1 || h->t0 < 0 || h->t0 >= T) return 0;
    return adv_ws_bytes((size_t)sc->NA, (size_t)T * h->base.scale, (size_t)h->base.P, (size_t)h->base.NE, (size_t)(T - h->t0),
                        (size_t)sc->B);
}

extern "C" int strive_adv_gen_fwd(const StriveScenes* sc, const StriveMap* map, const StriveAdvGen* h, const float* traj,
                                  const float* tgt, int32_t T, const float* z, const float* mu, const float* var, float* out,
                                  float* soft, float* rew, void* ws, size_t ws_bytes, strive_stream_t stream) {
    if (int rc = adv_check(sc, h, T)) return rc;
    STRIVE_CHECK_ARG(traj && tgt && out && soft && rew && ws && z && mu && var, "null argument");
    const StriveAvoidColl* hb = &h->base;
    if (hb->w_env > 0.f && hb->NE > 0) STRIVE_CHECK_ARG(map, "null map");
    const int NA = sc->NA, TO = T * hb->scale, NT = T - h->t0;
    STRIVE_CHECK_ARG(ws_bytes >= adv_ws_bytes(NA, TO, hb->P, hb->NE, NT, sc->B), "workspace too small");
    StriveArena ar(ws, ws_bytes);
    const AdvWs w = adv_layout(ar, NA, TO, hb->P, hb->NE, NT, sc->B);
    hipStream_t st = (hipStream_t)stream;
    const bool veh = (hb->w_veh > 0.f || h->w_plan > 0.f) && hb->P > 0;
    if (int rc = coll_forward_stages(sc, map, hb, traj, T, w.av, veh, /*cull=*/0, h->scene_alive, stream)) return rc;
    AdvArgs A = adv_args(sc, h, w, T, traj, tgt, z, mu, var);
    if (!veh) { A.a.w_veh = 0.f; A.w_plan = 0.f; }
    if (hb->NE == 0) A.a.w_env = 0.f;
    if (sc->B > 0) {
        hipLaunchKernelGGL(adv_crash_kernel, dim3(sc->B), dim3(256), 0, st, A);
        STRIVE_CHECK_LAUNCH();
    }
    const int nb = reduce_blocks(hb, TO);
    hipLaunchKernelGGL(loss_partial_kernel<true>, dim3(nb), dim3(256), 0, st, A, w.partial);
    STRIVE_CHECK_LAUNCH();
    hipLaunchKernelGGL(adv_final_kernel, dim3(1), dim3(64), 0, st, A, (const double*)w.partial, nb, w.sums, w.sel, out, soft, rew);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int strive_adv_gen_bwd(const StriveScenes* sc, const StriveAdvGen* h, const float* traj, const float* tgt, int32_t T,
                                  const float* z, const float* mu, const float* var, const float* d_loss, void* ws,
                                  size_t ws_bytes, float* d_traj, float* d_tgt, float* d_z, strive_stream_t stream) {
    if (int rc = adv_check(sc, h, T)) return rc;
    STRIVE_CHECK_ARG(traj && tgt && d_loss && ws && d_traj && d_tgt && d_z && z && mu && var, "null argument");
    const StriveAvoidColl* hb = &h->base;
    const int NA = sc->NA, TO = T * hb->scale, NT = T - h->t0;
    STRIVE_CHECK_ARG(ws_bytes >= adv_ws_bytes(NA, TO, hb->P, hb->NE, NT, sc->B), "workspace too small");
    if (NA == 0) return 0;
    StriveArena ar(ws, ws_bytes);
    const AdvWs w = adv_layout(ar, NA, TO, hb->P, hb->NE, NT, sc->B);
    hipStream_t st = (hipStream_t)stream;
    AdvArgs A = adv_args(sc, h, w, T, traj, tgt, z, mu, var);
    const bool veh = (hb->w_veh > 0.f || h->w_plan > 0.f) && hb->P > 0;
    if (hb->NE == 0) A.a.w_env = 0.f;
    const long long n = (long long)NA * TO + (long long)A.a.NZ * A.a.D;
    hipLaunchKernelGGL(loss_grad_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, hb->env_of_agent,
                       (const double*)w.sums, d_loss, w.av.d_fine, d_z);
    STRIVE_CHECK_LAUNCH();
    if (int rc = coll_backward_stages(sc, hb, w.av, w.sums, traj, T, d_loss, d_traj, stream, veh, h->slot_ne, w.rew_sel, h->w_plan))
        return rc;
    if (sc->B > 0) {
        hipLaunchKernelGGL(adv_crash_bwd_kernel, dim3(sc->B), dim3(256), 0, st, A, (const int32_t*)w.sel, (const double*)w.sums, d_loss, d_traj,
                           d_tgt);
        STRIVE_CHECK_LAUNCH();
    }
    return 0;
}
