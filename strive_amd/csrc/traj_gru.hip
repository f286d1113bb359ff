// GRU trajectory encoders (traj_encoder='gru', reference src/models/traffic_model.py:93-119, 453-523): a 4-layer, hidden-128
// nn.GRU over the T frames of every agent followed by Linear(128, 64) on the top layer's last state.
//
// One launch per encoder call: a workgroup owns a tile of TG_RB = 16 agent rows (one matrix-core row tile) and walks all T steps
// and all 4 layers with the four hidden states resident in LDS.  Both products of a layer-step (384 x in_l and 384 x 128) run on
// the matrix cores in the fp32-equivalent two-piece fp16 form (mlp_dev.h dense_mfma); the gates are fp32 VALU arithmetic with the
// helpers of rollout.hip's gru_layer_lds.  The layers of a step run one after the other (no layer wavefront): DESIGN.md 4.17.
//
// The kept forward also writes, per (step, layer, row), r | z | n | W_hn h + b_hn | h' (5 x 128 floats) and a copy of the input
// rows; the backward walks steps and layers in reverse with the recurrent adjoints in LDS, appends its (d gates, layer input)
// rows to the weight-gradient tapes (mlp_dev.h WJobTable) and one product per weight block follows the sweep.
#include "gnn_bwd_kernels.h"

#define TG_RB 16
#define TG_H STRIVE_TGRU_HID
#define TG_G (3 * STRIVE_TGRU_HID)
#define TG_L STRIVE_TGRU_LAYERS
#define TG_GLD 388      // leading dimension of the 384-wide gate buffers (padded, multiple of 4)
#define TG_XLD 36       // ... of the input rows (in_size <= 32)
#define TG_OLD 68       // ... of the 64-wide feature rows
#define TG_KROW (5 * TG_H)   // kept floats per (step, layer, row)
#define TG_KX 32        // kept floats per (row, step) of the input copy

struct TrajGRUDev {
    int in;
    const float* bih[TG_L];
    const float* bhh[TG_L];
    const uint4* wih_f[TG_L];
    const uint4* whh_f[TG_L];
    const uint4* wih_bf[TG_L][3];
    const uint4* whh_bf[TG_L][3];
    float ih_sc[TG_L], hh_sc[TG_L];
    const float* out_b;
    const uint4* out_wf;
    const uint4* out_wbf;
    float out_sc;
};

static inline TrajGRUDev traj_gru_dev(const StriveTrajGRU& g) {
    TrajGRUDev d;
    d.in = g.in_size;
    for (int l = 0; l < TG_L; ++l) {
        d.bih[l] = g.bih[l];
        d.bhh[l] = g.bhh[l];
        d.wih_f[l] = reinterpret_cast<const uint4*>(g.wih_f[l]);
        d.whh_f[l] = reinterpret_cast<const uint4*>(g.whh_f[l]);
        for (int q = 0; q < 3; ++q) {
            d.wih_bf[l][q] = reinterpret_cast<const uint4*>(g.wih_bf[l][q]);
            d.whh_bf[l][q] = reinterpret_cast<const uint4*>(g.whh_bf[l][q]);
        }
        d.ih_sc[l] = g.ih_sc[l];
        d.hh_sc[l] = g.hh_sc[l];
    }
    d.out_b = g.out_b;
    d.out_wf = reinterpret_cast<const uint4*>(g.out_wf);
    d.out_wbf = reinterpret_cast<const uint4*>(g.out_wbf);
    d.out_sc = g.out_sc;
    return d;
}

// gradients in named_parameters() order: per layer weight_ih | weight_hh | bias_ih | bias_hh, then the Linear's weight | bias
struct TrajGRUGradDev {
    float* wih[TG_L];
    float* whh[TG_L];
    float* bih[TG_L];
    float* bhh[TG_L];
    float* out_w;
    float* out_b;
};

static inline size_t traj_gru_param_count(int in) {
    size_t n = 0;
    for (int l = 0; l < TG_L; ++l) n += (size_t)TG_G * (l ? TG_H : in) + (size_t)TG_G * TG_H + 2 * TG_G;
    return n + (size_t)STRIVE_FEAT * TG_H + STRIVE_FEAT;
}

static inline TrajGRUGradDev traj_gru_grad_dev(int in, float* p) {
    TrajGRUGradDev g;
    for (int l = 0; l < TG_L; ++l) {
        g.wih[l] = p; p += (size_t)TG_G * (l ? TG_H : in);
        g.whh[l] = p; p += (size_t)TG_G * TG_H;
        g.bih[l] = p; p += TG_G;
        g.bhh[l] = p; p += TG_G;
    }
    g.out_w = p; p += (size_t)STRIVE_FEAT * TG_H;
    g.out_b = p;
    return g;
}

// kept buffer: [T][4][NA][TG_KROW] states, [NA][T][TG_KX] input rows, the job table, the weight-gradient tapes
struct TrajGRUKept {
    size_t states, xrows, table, tape, total;      // byte offsets / sizes
};
static inline size_t traj_gru_tape_floats(int in, size_t NA, size_t T) {
    size_t n = 0;
    for (int l = 0; l < TG_L; ++l) n += NA * T * (size_t)(2 * TG_G + (l ? TG_H : in) + TG_H);
    return n + NA * (size_t)(STRIVE_FEAT + TG_H);
}
static inline TrajGRUKept traj_gru_kept(int in, size_t NA, size_t T) {
    TrajGRUKept k;
    k.states = 0;
    k.xrows = strive_align_up(T * TG_L * NA * TG_KROW * 4, 256);
    k.table = k.xrows + strive_align_up(NA * T * TG_KX * 4, 256);
    k.tape = k.table + strive_align_up(sizeof(WJobTable), 256);
    k.total = k.tape + strive_align_up(traj_gru_tape_floats(in, NA, T) * 4, 256);
    return k;
}

// ---------------------------------------------------------------------------------------------
// forward: grid = ceil(NA / 16), 256 threads
// ---------------------------------------------------------------------------------------------
#define TG_FWD_LDS_FLOATS (TG_L * TG_RB * HLD + TG_RB * TG_XLD + 2 * TG_RB * TG_GLD + TG_RB * TG_OLD)

template <bool KEEP>
__global__ __launch_bounds__(256) void traj_gru_fwd_kernel(TrajGRUDev g, const float* __restrict__ x, int NA, int T,
                                                             float* __restrict__ feat, float* __restrict__ kstates,
                                                             float* __restrict__ kx) {
    HIP_DYNAMIC_SHARED(float, smem)
    float* s_h = smem;                              // [4][16][HLD]
    float* s_x = s_h + TG_L * TG_RB * HLD;          // [16][TG_XLD]
    float* s_gi = s_x + TG_RB * TG_XLD;             // [16][TG_GLD]
    float* s_gh = s_gi + TG_RB * TG_GLD;
    float* s_out = s_gh + TG_RB * TG_GLD;           // [16][TG_OLD]
    const int tid = threadIdx.x, r0 = blockIdx.x * TG_RB;
    const int nrows = (NA - r0) < TG_RB ? (NA - r0) : TG_RB;
    const int IN = g.in;
    for (int i = tid; i < TG_L * TG_RB * HLD; i += 256) s_h[i] = 0.f;
    for (int t = 0; t < T; ++t) {
        for (int i = tid; i < TG_RB * TG_KX; i += 256) {
            const int rr = i / TG_KX, k = i - rr * TG_KX;
            const float v = (rr < nrows && k < IN) ? x[((size_t)(r0 + rr) * T + t) * IN + k] : 0.f;
            s_x[rr * TG_XLD + k] = v;
            if (KEEP && rr < nrows) kx[((size_t)(r0 + rr) * T + t) * TG_KX + k] = v;
        }
        __syncthreads();
        for (int l = 0; l < TG_L; ++l) {
            float* h = s_h + l * TG_RB * HLD;
            const float* in = l ? s_h + (l - 1) * TG_RB * HLD : s_x;
            dense_mfma<TG_RB, false>(in, l ? HLD : TG_XLD, l ? TG_H : IN, g.wih_f[l], g.ih_sc[l], g.bih[l], s_gi, TG_GLD, TG_G, tid, 256);
            __syncthreads();
            dense_mfma<TG_RB, false>(h, HLD, TG_H, g.whh_f[l], g.hh_sc[l], g.bhh[l], s_gh, TG_GLD, TG_G, tid, 256);
            __syncthreads();
            for (int i = tid; i < TG_RB * TG_H; i += 256) {
                const int rr = i >> 7, c = i & (TG_H - 1);
                const float r = sigmoidf_(s_gi[rr * TG_GLD + c] + s_gh[rr * TG_GLD + c]);
                const float z = sigmoidf_(s_gi[rr * TG_GLD + TG_H + c] + s_gh[rr * TG_GLD + TG_H + c]);
                const float ghn = s_gh[rr * TG_GLD + 2 * TG_H + c];
                const float n = tanhf(s_gi[rr * TG_GLD + 2 * TG_H + c] + r * ghn);
                const float hn = (1.0f - z) * n + z * h[rr * HLD + c];
                h[rr * HLD + c] = hn;
                if (KEEP && rr < nrows) {
                    float* kq = kstates + (((size_t)t * TG_L + l) * NA + r0 + rr) * TG_KROW;
                    kq[c] = r;
                    kq[TG_H + c] = z;
                    kq[2 * TG_H + c] = n;
                    kq[3 * TG_H + c] = ghn;
                    kq[4 * TG_H + c] = hn;
                }
            }
            __syncthreads();
        }
    }
    dense_mfma<TG_RB, false>(s_h + (TG_L - 1) * TG_RB * HLD, HLD, TG_H, g.out_wf, g.out_sc, g.out_b, s_out, TG_OLD, STRIVE_FEAT, tid, 256);
    __syncthreads();
    for (int i = tid; i < nrows * STRIVE_FEAT; i += 256) {
        const int rr = i / STRIVE_FEAT, c = i - rr * STRIVE_FEAT;
        feat[(size_t)(r0 + rr) * STRIVE_FEAT + c] = s_out[rr * TG_OLD + c];
    }
}

// ---------------------------------------------------------------------------------------------
// backward: grid = ceil(NA / 16), 256 threads; weight gradients through the job table
// ---------------------------------------------------------------------------------------------
#define TG_BWD_LDS_FLOATS (TG_L * TG_RB * HLD + 3 * TG_RB * HLD + 2 * TG_RB * TG_GLD + TG_RB * TG_OLD)

__global__ __launch_bounds__(256) void traj_gru_bwd_kernel(TrajGRUDev g, TrajGRUGradDev gr, const float* __restrict__ kstates,
                                                             const float* __restrict__ kx, int NA, int T,
                                                             const float* __restrict__ d_feat, WJobTable* jobs) {
    HIP_DYNAMIC_SHARED(float, smem)
    float* s_dh = smem;                             // [4][16][HLD]  adjoint of every layer's state from the later steps
    float* s_dx = s_dh + TG_L * TG_RB * HLD;        // [16][HLD]     adjoint of this step's input of the layer above
    float* s_a = s_dx + TG_RB * HLD;                // [16][HLD]     layer input rows
    float* s_hp = s_a + TG_RB * HLD;                // [16][HLD]     previous state rows
    float* s_dgi = s_hp + TG_RB * HLD;              // [16][TG_GLD]
    float* s_dgh = s_dgi + TG_RB * TG_GLD;
    float* s_df = s_dgh + TG_RB * TG_GLD;           // [16][TG_OLD]
    const int tid = threadIdx.x, r0 = blockIdx.x * TG_RB;
    const int nrows = (NA - r0) < TG_RB ? (NA - r0) : TG_RB;
    const int IN = g.in;
    for (int i = tid; i < TG_L * TG_RB * HLD; i += 256) s_dh[i] = 0.f;
    for (int i = tid; i < TG_RB * TG_OLD; i += 256) {
        const int rr = i / TG_OLD, c = i - rr * TG_OLD;
        s_df[i] = (rr < nrows && c < STRIVE_FEAT) ? d_feat[(size_t)(r0 + rr) * STRIVE_FEAT + c] : 0.f;
    }
    for (int i = tid; i < TG_RB * TG_H; i += 256) {
        const int rr = i >> 7, c = i & (TG_H - 1);
        s_a[rr * HLD + c] = rr < nrows ? kstates[(((size_t)(T - 1) * TG_L + TG_L - 1) * NA + r0 + rr) * TG_KROW + 4 * TG_H + c] : 0.f;
    }
    __syncthreads();
    // the Linear: dW = d_feat^T h, adjoint of the top layer's last state
    wgrad_lds(s_df, TG_OLD, STRIVE_FEAT, s_a, HLD, TG_H, gr.out_w, TG_H, gr.out_b, nrows, tid, 256, jobs);
    dense_mfma<TG_RB, false>(s_df, TG_OLD, STRIVE_FEAT, g.out_wbf, g.out_sc, nullptr, s_dh + (TG_L - 1) * TG_RB * HLD, HLD, TG_H, tid, 256);
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        for (int l = TG_L - 1; l >= 0; --l) {
            float* dh = s_dh + l * TG_RB * HLD;
            const int AIN = l ? TG_H : IN;
            const float* kq0 = kstates + (((size_t)t * TG_L + l) * NA + r0) * TG_KROW;
            for (int i = tid; i < TG_RB * TG_H; i += 256) {
                const int rr = i >> 7, c = i & (TG_H - 1);
                const bool live = rr < nrows;
                const float hp = (live && t > 0) ? kstates[(((size_t)(t - 1) * TG_L + l) * NA + r0 + rr) * TG_KROW + 4 * TG_H + c] : 0.f;
                s_hp[rr * HLD + c] = hp;
                float a = 0.f;
                if (live) {
                    if (l) a = kstates[(((size_t)t * TG_L + l - 1) * NA + r0 + rr) * TG_KROW + 4 * TG_H + c];
                    else if (c < TG_KX) a = kx[((size_t)(r0 + rr) * T + t) * TG_KX + c];
                }
                s_a[rr * HLD + c] = a;
                float dar = 0.f, daz = 0.f, dan = 0.f, dghn = 0.f, dhz = 0.f;
                if (live) {
                    const float* kq = kq0 + (size_t)rr * TG_KROW;
                    const float r = kq[c], z = kq[TG_H + c], n = kq[2 * TG_H + c], ghn = kq[3 * TG_H + c];
                    const float d = dh[rr * HLD + c] + (l < TG_L - 1 ? s_dx[rr * HLD + c] : 0.f);
                    dan = d * (1.0f - z) * (1.0f - n * n);
                    daz = d * (hp - n) * z * (1.0f - z);
                    dar = dan * ghn * r * (1.0f - r);
                    dghn = dan * r;
                    dhz = d * z;
                }
                s_dgi[rr * TG_GLD + c] = dar;
                s_dgi[rr * TG_GLD + TG_H + c] = daz;
                s_dgi[rr * TG_GLD + 2 * TG_H + c] = dan;
                s_dgh[rr * TG_GLD + c] = dar;
                s_dgh[rr * TG_GLD + TG_H + c] = daz;
                s_dgh[rr * TG_GLD + 2 * TG_H + c] = dghn;
                dh[rr * HLD + c] = dhz;
            }
            __syncthreads();
            wgrad_lds(s_dgi, TG_GLD, TG_G, s_a, HLD, AIN, gr.wih[l], AIN, gr.bih[l], nrows, tid, 256, jobs);
            wgrad_lds(s_dgh, TG_GLD, TG_G, s_hp, HLD, TG_H, gr.whh[l], TG_H, gr.bhh[l], nrows, tid, 256, jobs);
            if (t > 0) {
                // adjoint of the previous state: dh z (above) + d gates_h W_hh, one product per gate block
                dense_mfma<TG_RB, true>(s_dgh, TG_GLD, TG_H, g.whh_bf[l][0], g.hh_sc[l], nullptr, dh, HLD, TG_H, tid, 256);
                __syncthreads();
                dense_mfma<TG_RB, true>(s_dgh + TG_H, TG_GLD, TG_H, g.whh_bf[l][1], g.hh_sc[l], nullptr, dh, HLD, TG_H, tid, 256);
                __syncthreads();
                dense_mfma<TG_RB, true>(s_dgh + 2 * TG_H, TG_GLD, TG_H, g.whh_bf[l][2], g.hh_sc[l], nullptr, dh, HLD, TG_H, tid, 256);
                __syncthreads();
            }
            if (l > 0) {
                // adjoint of this step's input = the state of the layer below
                dense_mfma<TG_RB, false>(s_dgi, TG_GLD, TG_H, g.wih_bf[l][0], g.ih_sc[l], nullptr, s_dx, HLD, TG_H, tid, 256);
                __syncthreads();
                dense_mfma<TG_RB, true>(s_dgi + TG_H, TG_GLD, TG_H, g.wih_bf[l][1], g.ih_sc[l], nullptr, s_dx, HLD, TG_H, tid, 256);
                __syncthreads();
                dense_mfma<TG_RB, true>(s_dgi + 2 * TG_H, TG_GLD, TG_H, g.wih_bf[l][2], g.ih_sc[l], nullptr, s_dx, HLD, TG_H, tid, 256);
                __syncthreads();
            }
            __syncthreads();      // the tape rows are copied before the next layer-step overwrites them
        }
    }
}

// ---------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------
static int traj_gru_check(const StriveTrajGRU* g, const char* fn, int32_t NA, int32_t T) {
    if (!g) { strive_set_error("%s: null descriptor", fn); return -1; }
    if (T < 1) { strive_set_error("%s: sequence length T = %d, need T >= 1", fn, (int)T); return -1; }
    if (g->in_size < 1 || g->in_size > STRIVE_TGRU_MAX_IN) {
        strive_set_error("%s: input width %d outside 1 .. %d", fn, (int)g->in_size, STRIVE_TGRU_MAX_IN);
        return -1;
    }
    if (NA < 0 || (size_t)NA * (size_t)T > 0x3fffffffull) { strive_set_error("%s: NA * T out of range", fn); return -1; }
    for (int l = 0; l < TG_L; ++l) {
        bool ok = g->wih[l] && g->whh[l] && g->bih[l] && g->bhh[l] && g->wih_f[l] && g->whh_f[l];
        for (int q = 0; q < 3; ++q) ok = ok && g->whh_bf[l][q] && (l == 0 || g->wih_bf[l][q]);
        if (!ok) { strive_set_error("%s: layer %d of the descriptor is incomplete", fn, l); return -1; }
    }
    if (!g->out_w || !g->out_b || !g->out_wf || !g->out_wbf) { strive_set_error("%s: output layer missing", fn); return -1; }
    return 0;
}

template <typename K>
static void traj_gru_lds_attr(K kernel, PerDeviceOnce& once, size_t bytes) {
    const int dev = once.device();
    if (!once.is_done(dev)) {
        (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        once.set_done(dev);
    }
}

extern "C" size_t strive_traj_gru_param_count(const StriveTrajGRU* gru) { return gru ? traj_gru_param_count(gru->in_size) : 0; }

extern "C" size_t strive_traj_gru_keep_bytes(const StriveTrajGRU* gru, int32_t NA, int32_t T) {
    if (!gru || NA < 0 || T < 1) return 0;
    return traj_gru_kept(gru->in_size, (size_t)NA, (size_t)T).total;
}

extern "C" int strive_traj_gru_fwd(const StriveTrajGRU* gru, const float* x, int32_t NA, int32_t T, float* feat,
                                   strive_stream_t stream) {
    if (traj_gru_check(gru, __func__, NA, T)) return -1;
    STRIVE_CHECK_ARG(x && feat, "null argument");
    if (NA == 0) return 0;
    static PerDeviceOnce once;
    traj_gru_lds_attr(traj_gru_fwd_kernel<false>, once, TG_FWD_LDS_FLOATS * 4);
    hipLaunchKernelGGL(traj_gru_fwd_kernel<false>, dim3((NA + TG_RB - 1) / TG_RB), dim3(256), TG_FWD_LDS_FLOATS * 4, (hipStream_t)stream,
                       traj_gru_dev(*gru), x, (int)NA, (int)T, feat, (float*)nullptr, (float*)nullptr);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int strive_traj_gru_fwd_keep(const StriveTrajGRU* gru, const float* x, int32_t NA, int32_t T, float* feat, void* kept,
                                        size_t kept_bytes, strive_stream_t stream) {
    if (traj_gru_check(gru, __func__, NA, T)) return -1;
    STRIVE_CHECK_ARG(x && feat && kept, "null argument");
    const TrajGRUKept k = traj_gru_kept(gru->in_size, (size_t)NA, (size_t)T);
    STRIVE_CHECK_ARG(kept_bytes >= k.total, "kept buffer too small");
    if (NA == 0) return 0;
    static PerDeviceOnce once;
    traj_gru_lds_attr(traj_gru_fwd_kernel<true>, once, TG_FWD_LDS_FLOATS * 4);
    char* kb = (char*)kept;
    hipLaunchKernelGGL(traj_gru_fwd_kernel<true>, dim3((NA + TG_RB - 1) / TG_RB), dim3(256), TG_FWD_LDS_FLOATS * 4, (hipStream_t)stream,
                       traj_gru_dev(*gru), x, (int)NA, (int)T, feat, (float*)(kb + k.states), (float*)(kb + k.xrows));
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int strive_traj_gru_bwd(const StriveTrajGRU* gru, int32_t NA, int32_t T, void* kept, size_t kept_bytes, const float* d_feat,
                                   float* d_params, strive_stream_t stream_) {
    if (traj_gru_check(gru, __func__, NA, T)) return -1;
    STRIVE_CHECK_ARG(kept && d_feat && d_params, "null argument");
    const TrajGRUKept k = traj_gru_kept(gru->in_size, (size_t)NA, (size_t)T);
    STRIVE_CHECK_ARG(kept_bytes >= k.total, "kept buffer too small");
    if (NA == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    char* kb = (char*)kept;
    WJobTable* jobs = (WJobTable*)(kb + k.table);
    float* tape = (float*)(kb + k.tape);
    const int in = gru->in_size;
    const TrajGRUGradDev gr = traj_gru_grad_dev(in, d_params);
    WJobsPlan plan;
    memset(&plan.t, 0, sizeof(plan.t));
    plan.tape_floats = 0; plan.max_in = 1; plan.max_out = 1;
    plan.dropped = false; plan.too_large = false;
    const int cap = NA * T;
    for (int l = 0; l < TG_L; ++l) {
        const int ain = l ? TG_H : in;
        wjobs_add(plan, tape, gr.wih[l], gr.bih[l], TG_G, ain, ain, cap);
        wjobs_add(plan, tape, gr.whh[l], gr.bhh[l], TG_G, TG_H, TG_H, cap);
    }
    wjobs_add(plan, tape, gr.out_w, gr.out_b, STRIVE_FEAT, TG_H, TG_H, NA);
    STRIVE_CHECK_ARG(!plan.dropped && plan.tape_floats == traj_gru_tape_floats(in, (size_t)NA, (size_t)T), "weight-gradient job plan");
    wjobs_finish(plan.t);
    hipLaunchKernelGGL(wjobs_upload_kernel, dim3(1), dim3(64), 0, stream, jobs, plan.t);
    static PerDeviceOnce once;
    traj_gru_lds_attr(traj_gru_bwd_kernel, once, TG_BWD_LDS_FLOATS * 4);
    hipLaunchKernelGGL(traj_gru_bwd_kernel, dim3((NA + TG_RB - 1) / TG_RB), dim3(256), TG_BWD_LDS_FLOATS * 4, stream, traj_gru_dev(*gru), gr,
                       (const float*)(kb + k.states), (const float*)(kb + k.xrows), (int)NA, (int)T, d_feat, jobs);
    hipLaunchKernelGGL(wjobs_gemm_kernel, dim3((plan.max_in + 63) / 64, (plan.max_out + 63) / 64, plan.t.ztotal), dim3(256), 0, stream, jobs);
    STRIVE_CHECK_LAUNCH();
    return 0;
}
