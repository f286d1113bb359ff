// Stand-alone MLP forward and scene-interaction-network forward (used by embed(): past/future encoders,
// prior and posterior networks), plus the three forward kernels the decoder rollout shares.
#include "gnn_bwd_kernels.h"

// ---------------------------------------------------------------------------------------------
// MLP forward on a (rows, F) matrix
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mlp_fwd_kernel(MLPDev m, const float* __restrict__ x, int rows,
                                                        float* __restrict__ y) {
    HIP_DYNAMIC_SHARED(float, smem)
    const int F = m.dims[0], O = m.dims[m.nlayers];
    const int in_ld = (F + 3) & ~3;
    float* s_in = smem;
    float* s_pre = s_in + RB_NODE * in_ld;
    float* s_act = s_pre + (STRIVE_MAX_LAYERS - 1) * RB_NODE * HLD;
    float* s_out = s_act + RB_NODE * HLD;
    const int tid = threadIdx.x, r0 = blockIdx.x * RB_NODE;
    FeatSrc f;
    f.n = 1;
    f.p[0] = x;
    f.w[0] = F;
    f.per_agent[0] = 0;
    gather_features<RB_NODE>(f, r0, rows, 1, s_in, in_ld, tid, 256);
    __syncthreads();
    mlp_forward_lds<RB_NODE>(m, s_in, in_ld, s_pre, s_act, s_out, HLD, false, tid, 256);
    for (int i = tid; i < RB_NODE * O; i += 256) {
        const int rr = i / O, c = i - rr * O;
        if (r0 + rr < rows) y[(size_t)(r0 + rr) * O + c] = s_out[rr * HLD + c];
    }
}

extern "C" int strive_mlp_fwd(const StriveMLP* mlp, const float* x, int32_t rows, float* y, strive_stream_t stream) {
    STRIVE_CHECK_ARG(mlp && x && y, "null argument");
    STRIVE_CHECK_ARG(mlp->nlayers >= 2 && mlp->nlayers <= STRIVE_MAX_LAYERS, "unsupported layer count");
    for (int l = 1; l < mlp->nlayers; ++l) STRIVE_CHECK_ARG(mlp->dims[l] == STRIVE_HID, "hidden width must be 128");
    STRIVE_CHECK_ARG(mlp->dims[mlp->nlayers] <= STRIVE_HID && mlp->dims[0] <= 512, "layer too wide");
    if (rows <= 0) return 0;
    const int in_ld = (mlp->dims[0] + 3) & ~3;
    const size_t lds = (size_t)(RB_NODE * in_ld + (STRIVE_MAX_LAYERS - 1) * RB_NODE * HLD + 2 * RB_NODE * HLD) * 4;
    hipLaunchKernelGGL(mlp_fwd_kernel, dim3((rows + RB_NODE - 1) / RB_NODE), dim3(256), lds, (hipStream_t)stream, mlp_dev(*mlp), x,
                       rows, y);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// MLP backward on a (rows, F) matrix: weight gradients (accumulated, flat named_parameters() order) and, optionally,
// the input gradient.  The forward is recomputed in LDS from x (nothing was saved).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mlp_bwd_kernel(MLPDev m, MLPGradDev gr, const float* __restrict__ x,
                                                        const float* __restrict__ dy, int rows, float* __restrict__ dx) {
    HIP_DYNAMIC_SHARED(float, smem)
    const int F = m.dims[0], O = m.dims[m.nlayers];
    const int in_ld = (F + 3) & ~3;
    float* s_in = smem;
    float* s_pre = s_in + RB_NODE * in_ld;
    float* s_act = s_pre + (STRIVE_MAX_LAYERS - 1) * RB_NODE * HLD;
    float* s_out = s_act + RB_NODE * HLD;
    float* s_go = s_out + RB_NODE * HLD;
    float* s_ga = s_go + RB_NODE * HLD;
    float* s_gb = s_ga + RB_NODE * HLD;
    float* s_din = s_gb + RB_NODE * HLD;     // [RB_NODE][in_ld]
    const int tid = threadIdx.x, r0 = blockIdx.x * RB_NODE;
    const int nrows = (rows - r0) < RB_NODE ? (rows - r0) : RB_NODE;
    FeatSrc f;
    f.n = 1;
    f.p[0] = x;
    f.w[0] = F;
    f.per_agent[0] = 0;
    gather_features<RB_NODE>(f, r0, rows, 1, s_in, in_ld, tid, 256);
    __syncthreads();
    mlp_forward_lds<RB_NODE>(m, s_in, in_ld, s_pre, s_act, s_out, HLD, false, tid, 256);
    for (int i = tid; i < RB_NODE * HLD; i += 256) {
        const int rr = i / HLD, c = i - rr * HLD;
        s_go[i] = (rr < nrows && c < O) ? dy[(size_t)(r0 + rr) * O + c] : 0.f;
    }
    __syncthreads();
    mlp_backward_lds<RB_NODE, true>(m, s_pre, s_go, HLD, s_ga, s_gb, dx ? s_din : nullptr, in_ld, false, tid, 256, &gr, s_act, s_in, in_ld,
                              nrows);
    if (dx) {
        for (int i = tid; i < RB_NODE * F; i += 256) {
            const int rr = i / F, c = i - rr * F;
            if (rr < nrows) dx[(size_t)(r0 + rr) * F + c] = s_din[rr * in_ld + c];
        }
    }
}

extern "C" size_t strive_mlp_param_count(const StriveMLP* mlp) { return mlp ? mlp_param_count(*mlp) : 0; }

extern "C" int strive_mlp_bwd(const StriveMLP* mlp, const float* x, const float* dy, int32_t rows, float* dx, float* d_params,
                              strive_stream_t stream) {
    STRIVE_CHECK_ARG(mlp && x && dy && d_params, "null argument");
    STRIVE_CHECK_ARG(mlp->nlayers >= 2 && mlp->nlayers <= STRIVE_MAX_LAYERS, "unsupported layer count");
    for (int l = 1; l < mlp->nlayers; ++l) STRIVE_CHECK_ARG(mlp->dims[l] == STRIVE_HID, "hidden width must be 128");
    STRIVE_CHECK_ARG(mlp->dims[mlp->nlayers] <= STRIVE_HID && mlp->dims[0] <= 512, "layer too wide");
    if (rows <= 0) return 0;
    const int in_ld = (mlp->dims[0] + 3) & ~3;
    const size_t lds = (size_t)(2 * RB_NODE * in_ld + (STRIVE_MAX_LAYERS - 1) * RB_NODE * HLD + 5 * RB_NODE * HLD) * 4;
    float* p = d_params;
    const MLPGradDev gr = mlp_grad_dev(*mlp, &p);
    hipLaunchKernelGGL(mlp_bwd_kernel, dim3((rows + RB_NODE - 1) / RB_NODE), dim3(256), lds, (hipStream_t)stream, mlp_dev(*mlp), gr,
                       x, dy, rows, dx);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// SceneInteractionNet forward
// ---------------------------------------------------------------------------------------------
extern "C" size_t strive_gnn_workspace_bytes(const StriveGNN* gnn, const StriveScenes* sc) {
    if (!gnn || !sc) return 0;
    const size_t R = (size_t)sc->NA * sc->NS;
    size_t b = 0;
    b += strive_align_up(R * gnn->D * 4, 256);          // X
    b += 2 * strive_align_up(R * STRIVE_HID * 4, 256);  // P, Q
    b += strive_align_up(R * gnn->D * 4, 256);          // A
    b += strive_align_up(R * gnn->D * 4, 256);          // ARG
    return b;
}

extern "C" int strive_gnn_fwd(const StriveGNN* gnn, const StriveScenes* sc, const float* x, const float* pos,
                              const float* sem, float* out, void* ws, size_t ws_bytes, strive_stream_t stream) {
    STRIVE_CHECK_ARG(gnn && sc && x && pos && sem && out && ws, "null argument");
    STRIVE_CHECK_ARG(ws_bytes >= strive_gnn_workspace_bytes(gnn, sc), "workspace too small");
    const int R = sc->NA * sc->NS;
    if (R == 0) return 0;
    StriveArena ar(ws, ws_bytes);
    GnnBuffers gb;
    gb.X = ar.take<float>((size_t)R * gnn->D);
    gb.P = ar.take<float>((size_t)R * STRIVE_HID);
    gb.Q = ar.take<float>((size_t)R * STRIVE_HID);
    gb.A = ar.take<float>((size_t)R * gnn->D);
    gb.ARG = ar.take<int32_t>((size_t)R * gnn->D);
    gb.PRE_IN = nullptr;
    gb.PRE_E = nullptr;
    FeatSrc f;
    f.n = 1;
    f.p[0] = x;
    f.w[0] = gnn->mlp_in.dims[0];
    f.per_agent[0] = 0;
    int rc = gnn_forward_launch(*gnn, *sc, f, pos, sem, gb, out, (hipStream_t)stream);
    if (rc) return rc;
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// SceneInteractionNet backward: d_out -> dx (input features) and the weight gradients (accumulated, flat
// named_parameters() order).  The forward is recomputed (node embeddings, partials, aggregates) into the workspace.
// ---------------------------------------------------------------------------------------------
// deferred weight gradients of the stand-alone backward (round 5; the rollout's sweep has had them since round 3): every kernel
// appends its (adjoint, input) rows to per-block tapes and ONE product per block follows -- with atomics straight into dW a
// 64-row call spent 450 us in three kernels (141 + 163 + 152), most of it in 64 atomic wave instructions per layer and workgroup
static WJobsPlan gnn_bwd_plan(const StriveGNN& g, const StriveScenes& sc, float* d_params, float* tape) {
    WJobsPlan p;
    memset(&p.t, 0, sizeof(p.t));
    p.tape_floats = 0; p.max_in = 1; p.max_out = 1;
    p.dropped = false; p.too_large = false;
    const size_t R = (size_t)sc.NA * sc.NS;
    const size_t edges = sc.n_edges > 0 ? (size_t)sc.n_edges : R * (size_t)(sc.max_n > 1 ? sc.max_n : 1);
    p.too_large = R > 0x7fffffffull || edges > 0x7fffffffull;
    const GNNGradDev gr = gnn_grad_dev(g, d_params);
    wjobs_add_gnn(p, tape, g, gr, p.too_large ? 1 : (int)(R > 0 ? R : 1), p.too_large ? 1 : (int)(edges > 0 ? edges : 1));
    wjobs_finish(p.t);
    return p;
}

extern "C" size_t strive_gnn_bwd_workspace_bytes(const StriveGNN* gnn, const StriveScenes* sc) {
    if (!gnn || !sc) return 0;
    const size_t R = (size_t)sc->NA * sc->NS;
    float* fake = reinterpret_cast<float*>(uintptr_t(1) << 20);      // (planning only: nothing is dereferenced)
    const size_t tape = gnn_bwd_plan(*gnn, *sc, fake, fake).tape_floats;
    return strive_gnn_workspace_bytes(gnn, sc) + strive_measure([&](StriveArena& a) { gnn_bwd_buffers_take(a, R, gnn->D, sc->max_n > 0 ? sc->max_n : 1); }) +
           strive_align_up(R * 4 * 4, 256) + strive_align_up(sizeof(WJobTable), 256) + strive_align_up(tape * 4, 256) + 4096;
}

extern "C" int strive_gnn_bwd(const StriveGNN* gnn, const StriveScenes* sc, const float* x, const float* pos, const float* sem,
                              const float* d_out, float* dx, float* d_params, void* ws, size_t ws_bytes,
                              strive_stream_t stream_) {
    STRIVE_CHECK_ARG(gnn && sc && x && pos && sem && d_out && dx && d_params && ws, "null argument");
    STRIVE_CHECK_ARG(ws_bytes >= strive_gnn_bwd_workspace_bytes(gnn, sc), "workspace too small");
    STRIVE_CHECK_ARG(sc->max_n >= 1, "max_n not set");
    if (gnn_check(*gnn)) return -1;
    const int R = sc->NA * sc->NS;
    if (R == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    StriveArena ar(ws, ws_bytes);
    GnnBuffers gb;
    gb.X = ar.take<float>((size_t)R * gnn->D);
    gb.P = ar.take<float>((size_t)R * STRIVE_HID);
    gb.Q = ar.take<float>((size_t)R * STRIVE_HID);
    gb.A = ar.take<float>((size_t)R * gnn->D);
    gb.ARG = ar.take<int32_t>((size_t)R * gnn->D);
    gb.PRE_IN = nullptr;
    gb.PRE_E = nullptr;
    GnnBwdBuffers bw = gnn_bwd_buffers_take(ar, (size_t)R, gnn->D, sc->max_n);
    float* g_pos = ar.take<float>((size_t)R * 4);
    WJobTable* jobs = ar.take<WJobTable>(1);
    float* fake = reinterpret_cast<float*>(uintptr_t(1) << 20);
    float* wtape = ar.take<float>(gnn_bwd_plan(*gnn, *sc, fake, fake).tape_floats);
    STRIVE_CHECK_ARG(ar.ok(), "workspace arena overflow");
    FeatSrc f;
    f.n = 1;
    f.p[0] = x;
    f.w[0] = gnn->mlp_in.dims[0];
    f.per_agent[0] = 0;
    int rc = gnn_forward_launch(*gnn, *sc, f, pos, sem, gb, nullptr, stream);      // node1 + edge: X, P, Q, A, ARG
    if (rc) return rc;
    const GNNDev gd = gnn_dev(*gnn);
    GNNGradDev gr = gnn_grad_dev(*gnn, d_params);
    const bool atomics_only = strive_tuning().wgrad_atomics != 0;      // A/B switch: no deferred weight gradients
    WJobsPlan plan = gnn_bwd_plan(*gnn, *sc, d_params, wtape);
    const bool deferred = !atomics_only && !plan.too_large && !plan.dropped && plan.t.n > 0;
    if (deferred) {
        hipLaunchKernelGGL(wjobs_upload_kernel, dim3(1), dim3(64), 0, stream, jobs, plan.t);
        gr.mlp_in.jobs = gr.edge.jobs = gr.update.jobs = gr.mlp_out.jobs = jobs;
    }
    const ScenesDev sd = scenes_dev(*sc);
    const int in_ld1 = ld4(gnn->mlp_in.dims[0]), xs_ld = ld4(gnn->D + gnn->NC), in_ld2 = ld4(2 * gnn->D + gnn->NC);
    const int nb = (R + RB_NODE - 1) / RB_NODE;
    hipLaunchKernelGGL(gnn_node2_bwd_kernel, dim3(nb), dim3(256), gnn_node2_bwd_lds_bytes(in_ld2), stream, gd, gr, sc->NS, sem, gb,
                       d_out, bw.dX, bw.dA, R);
    EdgeBwdArgs ae;
    ae.dA = bw.dA; ae.ARG = gb.ARG; ae.dP = bw.dP; ae.DE1 = bw.DE1; ae.DPJ = bw.DPJ; ae.gpos_tgt = bw.gpos_tgt;
    hipLaunchKernelGGL(edge_bwd_kernel<true>, dim3((unsigned)R), dim3(256), edge_bwd_lds_bytes(), stream, gd, gr, sd, pos, gb, ae);
    Node1BwdArgs a1;
    a1.t = 0; a1.R = R; a1.dX = bw.dX; a1.dP = bw.dP; a1.DE1 = bw.DE1; a1.DPJ = bw.DPJ; a1.gpos_tgt = bw.gpos_tgt;
    a1.sem = sem; a1.PRE_IN = nullptr; a1.X = gb.X; a1.g_pos = g_pos; a1.g_full = dx; a1.g_pf = nullptr; a1.g_mf = nullptr; a1.dz = nullptr;
    hipLaunchKernelGGL(node1_bwd_kernel<true>, dim3(nb), dim3(256), node1_bwd_lds_bytes(in_ld1, xs_ld), stream, gd, gr, sd, f, a1);
    if (deferred)
        hipLaunchKernelGGL(wjobs_gemm_kernel, dim3((plan.max_in + 63) / 64, (plan.max_out + 63) / 64, plan.t.ztotal), dim3(256), 0, stream,
                           jobs);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Weight pack of one Linear layer in one launch (the training step re-packs every layer after the optimiser step; as torch
// tensor ops that was ~22 launches per layer): w (M, K) fp32 ->
//   wt  (K, M) fp32                                   the transpose the vector-ALU path streams
//   wf  fragments of  w  * scale                      [row tile][k-step][piece][lane][8 x fp16]   (StriveMLP.wf)
//   wbf fragments of  w^T * scale                     the same layout for the transposed matrix   (StriveMLP.wbf)
// with the two-piece split of strive_hip.h: p0 = fp16(v) to nearest even, p1 = fp16(v - p0).  Any output may be null.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack_split8(const float v[8], uint4& p0, uint4& p1) {
    uint32_t h[8], l[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const _Float16 a = (_Float16)v[i];
        const _Float16 c = (_Float16)(v[i] - (float)a);
        uint16_t ab, cb;
        __builtin_memcpy(&ab, &a, 2);
        __builtin_memcpy(&cb, &c, 2);
        h[i] = ab;
        l[i] = cb;
    }
    p0 = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    p1 = make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
}

// fragments of the (R, C) matrix a[r][c] = src[r * rs + c * cs]; thread = (tile, step, lane): both pieces
__device__ __forceinline__ void pack_fragments(const float* __restrict__ src, int R, int C, int rs, int cs, float scale,
                                               uint4* __restrict__ out, int idx) {
    const int KS = (C + 31) / 32;
    const int lane = idx & 63, t1 = idx >> 6;
    const int step = t1 % KS, tile = t1 / KS;
    const int r = tile * 16 + (lane & 15), c0 = step * 32 + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (r < R && c0 + j < C) ? src[(size_t)r * rs + (size_t)(c0 + j) * cs] * scale : 0.f;
    uint4 p0, p1;
    pack_split8(v, p0, p1);
    uint4* o = out + ((size_t)(tile * KS + step) * 2) * 64 + lane;
    o[0] = p0;
    o[64] = p1;
}

static __global__ __launch_bounds__(256) void pack_dense_kernel(const float* __restrict__ w, int M, int K, float scale,
                                                                  float* __restrict__ wt, uint4* __restrict__ wf, uint4* __restrict__ wbf) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int nf = ((M + 15) / 16) * ((K + 31) / 32) * 64, nb = ((K + 15) / 16) * ((M + 31) / 32) * 64;
    if (wf && idx < nf) pack_fragments(w, M, K, K, 1, scale, wf, idx);
    if (wbf && idx < nb) pack_fragments(w, K, M, 1, K, scale, wbf, idx);
    if (wt && idx < M * K) {
        const int k = idx / M, m = idx - k * M;
        wt[idx] = w[(size_t)m * K + k];
    }
}

// Any fragment table as ONE gather: out[i] = piece p of fp16-split(w[e] * scale) with (p, e) = (idx[i] / n_w, idx[i] % n_w), or 0
// where idx[i] == 2 n_w (the layout's zero slot).  The index table is the layout (params.py builds it once per shape).
static __global__ __launch_bounds__(256) void pack_split_gather_kernel(const float* __restrict__ w, int n_w, const int32_t* __restrict__ idx,
                                                                         int n_out, float scale, uint16_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int src = idx[i];
    uint16_t bits = 0;
    if (src >= 0 && src < 2 * n_w) {
        const int piece = src >= n_w ? 1 : 0;
        const float v = w[src - piece * n_w] * scale;
        const _Float16 a = (_Float16)v;
        const _Float16 c = piece ? (_Float16)(v - (float)a) : a;
        __builtin_memcpy(&bits, &c, 2);
    }
    out[i] = bits;
}

extern "C" int strive_pack_split_gather(const float* w, int32_t n_w, const int32_t* idx, int32_t n_out, float scale, void* out,
                                        strive_stream_t stream) {
    STRIVE_CHECK_ARG(w && idx && out && n_w > 0 && n_out >= 0 && n_w < (1 << 30), "bad argument");
    if (n_out == 0) return 0;
    hipLaunchKernelGGL(pack_split_gather_kernel, dim3((n_out + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, (int)n_w, idx, (int)n_out,
                       scale, (uint16_t*)out);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int strive_pack_dense(const float* w, int32_t M, int32_t K, float scale, float* wt, void* wf, void* wbf,
                                 strive_stream_t stream) {
    STRIVE_CHECK_ARG(w && M > 0 && K > 0, "bad argument");
    const int nf = ((M + 15) / 16) * ((K + 31) / 32) * 64, nb = ((K + 15) / 16) * ((M + 31) / 32) * 64;
    int n = M * K;
    n = nf > n ? nf : n;
    n = nb > n ? nb : n;
    hipLaunchKernelGGL(pack_dense_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, M, K, scale, wt, (uint4*)wf,
                       (uint4*)wbf);
    STRIVE_CHECK_LAUNCH();
    return 0;
}
