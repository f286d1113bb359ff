// Lane graphs built on the device: discretised lanes + lane connectivity -> the lane-graph tables of the reference
// (reference src/datasets/nuscenes_utils.py:28-122: remove_duplicates, process_lanegraph, process_edges; the Singapore flip of
//  src/datasets/map_env.py:131-144) and the tables the rule-based planner reads (StrivePlannerMap: connection records, CSR
//  lists, the edge table and the uniform grid over the edges, strive_amd/planners/hardcode_goalcond_nusc.py edge_grid).
//
// THE LENGTH RULE of this file (stated once in include/strive_hip.h, used for every distance below -- the duplicate test, the
// trimming test, the edge table and the connection lengths):        |(dx, dy)| = sqrt(fma(dy, dy, dx * dx))
// which is what numpy's np.linalg.norm of a 1-D pair evaluates (BLAS ddot accumulates with a fused multiply-add); the fixture
// tests/golden/g25_lane_graph.npz agrees with it on all 804 edge lengths, with the unfused sum on 751.
//
// Everything else is float64 with no contraction.  Integer prefix sums and min / max reductions are the only cross-thread
// combinations, so every output is independent of the launch geometry and identical from run to run; the one place where an
// atomic's order could show (the fill of a grid cell's edge list) is followed by a sort of that list.
//
// Protocol: sizes are unknown before they are counted, so both builders are a count call, ONE read-back of a small record by
// the host (sizes + refusal status), and a fill call into arrays of exactly those sizes.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TB = 256;                 // threads of every workgroup in this file
constexpr int SI = 4;                   // scan: items per thread
constexpr int ST = TB * SI;             // scan: items per workgroup
constexpr int NONE = 0x7fffffff;

__device__ __forceinline__ double lg_len(double dx, double dy) { return sqrt(fma(dy, dy, dx * dx)); }

inline int blocks_for(long long n, int per) { return (int)((n + per - 1) / per); }

// ---- exclusive prefix sum of n int32 (out has n + 1 entries, out[n] = total); sums: one int per tile of ST items ----------
__global__ __launch_bounds__(TB) void scan_tile_sums(const int* __restrict__ in, int n, int* __restrict__ sums) {
    __shared__ int s[TB];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * ST + (long long)tid * SI;
    int v = 0;
    for (int k = 0; k < SI; ++k) if (base + k < n) v += in[base + k];
    s[tid] = v;
    __syncthreads();
    for (int off = TB / 2; off > 0; off >>= 1) {
        if (tid < off) s[tid] += s[tid + off];
        __syncthreads();
    }
    if (tid == 0) sums[blockIdx.x] = s[0];
}

// inclusive scan of one int per thread over the workgroup (Hillis-Steele in LDS)
__device__ __forceinline__ int block_inclusive_scan(int v, int* s) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < TB; off <<= 1) {
        const int add = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    return s[tid];
}

__global__ __launch_bounds__(TB) void scan_sums(int* __restrict__ sums, int nb) {      // one workgroup: in place, exclusive
    __shared__ int s[TB];
    const int tid = threadIdx.x;
    const int chunk = (nb + TB - 1) / TB;
    const int a = tid * chunk, b = (a + chunk < nb) ? a + chunk : nb;
    int v = 0;
    for (int i = a; i < b; ++i) v += sums[i];
    int run = block_inclusive_scan(v, s) - v;
    for (int i = a; i < b; ++i) {
        const int t = sums[i];
        sums[i] = run;
        run += t;
    }
}

__global__ __launch_bounds__(TB) void scan_apply(const int* __restrict__ in, int n, const int* __restrict__ sums, int* __restrict__ out) {
    __shared__ int s[TB];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * ST + (long long)tid * SI;
    int item[SI], v = 0;
    for (int k = 0; k < SI; ++k) {
        item[k] = (base + k < n) ? in[base + k] : 0;
        v += item[k];
    }
    int run = sums[blockIdx.x] + block_inclusive_scan(v, s) - v;
    for (int k = 0; k < SI; ++k) {
        if (base + k < n) {
            out[base + k] = run;
            run += item[k];
            if (base + k == n - 1) out[n] = run;
        }
    }
}

int exclusive_scan(const int* in, int n, int* out, int* sums, hipStream_t st) {
    const int nb = blocks_for(n, ST);
    hipLaunchKernelGGL(scan_tile_sums, dim3(nb), dim3(TB), 0, st, in, n, sums);
    hipLaunchKernelGGL(scan_sums, dim3(1), dim3(TB), 0, st, sums, nb);
    hipLaunchKernelGGL(scan_apply, dim3(nb), dim3(TB), 0, st, in, n, (const int*)sums, out);
    return 0;
}

// ---- lane graph --------------------------------------------------------------------------------------------------------------
struct LgWork {                 // the count call's products, kept for the fill (all int32, P = points, NL = lanes)
    int* keep;                  // (P)     rule 1: 1 = the point survives remove_duplicates
    int* rank;                  // (P+1)   exclusive prefix of keep
    int* lane_n;                // (NL)    nodes of the lane after rule 2
    int* node_start;            // (NL+1)  first node of the lane
    int* node_src;              // (P)     node -> point
    int* node_lane;             // (P)     node -> lane
    int* out_deg;               // (P)
    int* in_deg;                // (P)
    int* succ_ptr;              // (P+1)   exclusive prefix of out_deg (entries past N repeat the total)
    int* pred_ptr;              // (P+1)
    int* sums;                  // scan scratch
    int* first;                 // (4)     lowest offending lane (rules 1, 2) / node (rules 3, 4) of each refusal, NONE = none
};

size_t lg_work_ints(int NL, int P) {
    const size_t big = (size_t)(P > NL ? P : NL);
    return (size_t)P * 8 + 3 + (size_t)NL * 2 + 1 + (big / ST + 2) + 4;      // lg_carve's arrays, in its order
}

LgWork lg_carve(void* ws, int NL, int P) {
    LgWork w;
    int* p = (int*)ws;
    w.keep = p; p += P;
    w.rank = p; p += P + 1;
    w.lane_n = p; p += NL;
    w.node_start = p; p += NL + 1;
    w.node_src = p; p += P;
    w.node_lane = p; p += P;
    w.out_deg = p; p += P;
    w.in_deg = p; p += P;
    w.succ_ptr = p; p += P + 1;
    w.pred_ptr = p; p += P + 1;
    const size_t big = (size_t)(P > NL ? P : NL);
    w.sums = p; p += big / ST + 2;
    w.first = p;
    return w;
}

__device__ __forceinline__ int lane_of_point(const int* __restrict__ lane_ptr, int NL, int i) {
    int lo = 0, hi = NL;                           // the last l with lane_ptr[l] <= i (empty lanes repeat an offset)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (lane_ptr[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(TB) void lg_init(int* first) {
    if (threadIdx.x < 4) first[threadIdx.x] = NONE;
}

// rule 1 (remove_duplicates, :28-41): point i < n-1 of its lane is kept iff |p[i+1] - p[i]| > eps, the last one always
__global__ __launch_bounds__(TB) void lg_keep(StriveLaneGraphIn in, LgWork w) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= in.P) return;
    const int l = lane_of_point(in.lane_ptr, in.NL, i);
    const int a = in.lane_ptr[l], b = in.lane_ptr[l + 1];
    int k = 1;
    if (i + 1 < b) {
        const double dx = in.pts[2 * (i + 1)] - in.pts[2 * i], dy = in.pts[2 * (i + 1) + 1] - in.pts[2 * i + 1];
        k = lg_len(dx, dy) > in.eps ? 1 : 0;
    }
    w.keep[i] = k;
    if (i == a && !k) atomicMin(&w.first[0], l);
}

// rule 2 (:72-78): walk the lane's outgoing list; a successor whose FIRST point (never changed by this rule) lies within eps of
// this lane's present last point costs this lane that point
__global__ __launch_bounds__(TB) void lg_trim(StriveLaneGraphIn in, LgWork w) {
    const int l = blockIdx.x * TB + threadIdx.x;
    if (l >= in.NL) return;
    const int a = in.lane_ptr[l], b = in.lane_ptr[l + 1];
    int n = w.rank[b] - w.rank[a];
    int last = b - 1;                                                   // kept by rule 1 whenever the lane has a point
    bool emptied = n < 1;
    for (int j = in.out_ptr[l]; j < in.out_ptr[l + 1] && !emptied; ++j) {
        const int o = in.out_idx[j];
        if (o < 0 || o >= in.NL) continue;
        int f = in.lane_ptr[o];
        const int fe = in.lane_ptr[o + 1];
        while (f < fe && !w.keep[f]) ++f;                               // the successor's first point after rule 1
        if (f >= fe) continue;
        const double dx = in.pts[2 * f] - in.pts[2 * last], dy = in.pts[2 * f + 1] - in.pts[2 * last + 1];
        if (lg_len(dx, dy) <= in.eps) {
            --n;
            if (n < 1) { emptied = true; break; }
            --last;
            while (last > a && !w.keep[last]) --last;
        }
    }
    if (emptied) {
        n = 0;
        atomicMin(&w.first[1], l);
    }
    w.lane_n[l] = n;
}

__global__ __launch_bounds__(TB) void lg_nodes(StriveLaneGraphIn in, LgWork w) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= in.P || !w.keep[i]) return;
    const int l = lane_of_point(in.lane_ptr, in.NL, i);
    const int t = w.rank[i] - w.rank[in.lane_ptr[l]];
    if (t >= w.lane_n[l]) return;                                       // trimmed by rule 2
    const int v = w.node_start[l] + t;
    w.node_src[v] = i;
    w.node_lane[v] = l;
}

// Connection targets of node v in the reference's list order (:86-98).  Interior link first; on a lane's last node its present
// outgoing lanes' first nodes, on its first node its present incoming lanes' last nodes.
struct NodeCtx { int l, t, n; };
__device__ __forceinline__ NodeCtx node_ctx(const LgWork& w, int v) {
    NodeCtx c;
    c.l = w.node_lane[v];
    c.t = v - w.node_start[c.l];
    c.n = w.lane_n[c.l];
    return c;
}
template <typename F> __device__ __forceinline__ int for_each_succ(const StriveLaneGraphIn& in, const LgWork& w, int v, const NodeCtx& c, F f) {
    int k = 0;
    if (c.t < c.n - 1) f(k++, v + 1);
    else
        for (int j = in.out_ptr[c.l]; j < in.out_ptr[c.l + 1]; ++j) {
            const int o = in.out_idx[j];
            if (o >= 0 && o < in.NL) f(k++, w.node_start[o]);
        }
    return k;
}
template <typename F> __device__ __forceinline__ int for_each_pred(const StriveLaneGraphIn& in, const LgWork& w, int v, const NodeCtx& c, F f) {
    int k = 0;
    if (c.t >= 1) f(k++, v - 1);
    else
        for (int j = in.in_ptr[c.l]; j < in.in_ptr[c.l + 1]; ++j) {
            const int o = in.in_idx[j];
            if (o >= 0 && o < in.NL) f(k++, w.node_start[o] + w.lane_n[o] - 1);
        }
    return k;
}

// degrees of every node + the two refusals of process_edges (:106-122): an edge not longer than eps, a node pair listed twice
__global__ __launch_bounds__(TB) void lg_degrees(StriveLaneGraphIn in, LgWork w) {
    const int v = blockIdx.x * TB + threadIdx.x;
    if (v >= in.P) return;
    int od = 0, id = 0;
    if (w.first[0] == NONE && w.first[1] == NONE && v < w.node_start[in.NL]) {        // (a refused map has no valid numbering)
        const NodeCtx c = node_ctx(w, v);
        const int p = w.node_src[v];
        const double x0 = in.pts[2 * p], y0 = in.pts[2 * p + 1];
        bool is_short = false, twice = false;
        od = for_each_succ(in, w, v, c, [&](int k, int u) {
            const int q = w.node_src[u];
            if (!(lg_len(in.pts[2 * q] - x0, in.pts[2 * q + 1] - y0) > in.eps)) is_short = true;
            int kk = 0;
            for_each_succ(in, w, v, c, [&](int k2, int u2) { if (k2 < k && u2 == u) kk = 1; });
            if (kk) twice = true;
        });
        id = for_each_pred(in, w, v, c, [&](int, int) {});
        if (is_short) atomicMin(&w.first[2], v);
        if (twice) atomicMin(&w.first[3], v);
    }
    w.out_deg[v] = od;
    w.in_deg[v] = id;
}

__global__ void lg_counts(StriveLaneGraphIn in, LgWork w, int* __restrict__ counts) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    // the reference's order: every lane's rule 1, then every lane's rule 2, then the edges in node order (a node that trips both
    // edge rules is reported with the length rule)
    int status = 0, index = -1;
    if (w.first[0] != NONE) { status = STRIVE_LANE_GRAPH_FIRST_POINT_DROPPED; index = w.first[0]; }
    else if (w.first[1] != NONE) { status = STRIVE_LANE_GRAPH_LANE_EMPTIED; index = w.first[1]; }
    else if (w.first[2] != NONE && w.first[2] <= w.first[3]) { status = STRIVE_LANE_GRAPH_SHORT_EDGE; index = w.first[2]; }
    else if (w.first[3] != NONE) { status = STRIVE_LANE_GRAPH_EDGE_TWICE; index = w.first[3]; }
    counts[0] = w.node_start[in.NL];
    counts[1] = w.succ_ptr[in.P];
    counts[2] = w.pred_ptr[in.P];
    counts[3] = status;
    counts[4] = index;
    counts[5] = (status == STRIVE_LANE_GRAPH_SHORT_EDGE || status == STRIVE_LANE_GRAPH_EDGE_TWICE) ? w.node_lane[index] : index;   // the lane
    counts[6] = counts[7] = 0;
}

__global__ __launch_bounds__(TB) void lg_fill(StriveLaneGraphIn in, LgWork w, StriveLaneGraphOut out) {
    const int v = blockIdx.x * TB + threadIdx.x;
    if (v >= out.N) return;
    const NodeCtx c = node_ctx(w, v);
    const double H = in.height;
    const bool flip = in.flip != 0;
    const int p = w.node_src[v];
    const double x0 = in.pts[2 * p], y0 = in.pts[2 * p + 1];
    const double fy0 = flip ? H - y0 : y0;                        // xy[:,1] = H - y (map_env.py:138)
    out.xy[2 * v] = x0;
    out.xy[2 * v + 1] = fy0;
    const int sp = w.succ_ptr[v], pp = w.pred_ptr[v];
    out.succ_ptr[v] = sp;
    out.pred_ptr[v] = pp;
    if (v == out.N - 1) {
        out.succ_ptr[out.N] = w.succ_ptr[out.N];
        out.pred_ptr[out.N] = w.pred_ptr[out.N];
    }
    StriveLaneNode rs, rp;
    for (int k = 0; k < 4; ++k) { rs.node[k] = rp.node[k] = 0; rs.len[k] = rp.len[k] = 0.0; }
    for (int k = 0; k < 3; ++k) rs.pad[k] = rp.pad[k] = 0;
    // the planner's lengths come from the FINAL positions (after the flip): |xy[u] - xy[v]|
    auto final_len = [&](int u) {
        const int q = w.node_src[u];
        const double yq = in.pts[2 * q + 1];
        return lg_len(in.pts[2 * q] - x0, (flip ? H - yq : yq) - fy0);
    };
    rs.n = for_each_succ(in, w, v, c, [&](int k, int u) {
        const double ln = final_len(u);
        if (k < 4) { rs.node[k] = u; rs.len[k] = ln; }
        if (sp + k < out.M) {
            out.succ_idx[sp + k] = u;
            out.succ_len[sp + k] = ln;
            // process_edges (:106-122) on the positions BEFORE the flip, then edges[:,1] = H - y0, edges[:,3] *= -1 (:141-143)
            const int q = w.node_src[u];
            const double dx = in.pts[2 * q] - x0, dy = in.pts[2 * q + 1] - y0;
            const double d = lg_len(dx, dy);
            double* e = out.edges + 5 * (size_t)(sp + k);
            const double uy = dy / d;
            e[0] = x0; e[1] = fy0; e[2] = dx / d; e[3] = flip ? uy * -1.0 : uy; e[4] = d;
            out.edge_ix[2 * (size_t)(sp + k)] = v;
            out.edge_ix[2 * (size_t)(sp + k) + 1] = u;
        }
    });
    rp.n = for_each_pred(in, w, v, c, [&](int k, int u) {
        const double ln = final_len(u);
        if (k < 4) { rp.node[k] = u; rp.len[k] = ln; }
        if (pp + k < out.MI) {
            out.pred_idx[pp + k] = u;
            out.pred_len[pp + k] = ln;
        }
    });
    out.succ[v] = rs;
    out.pred[v] = rp;
}

// ---- edge grid ---------------------------------------------------------------------------------------------------------------
struct EdgeBox { double lox, loy, hix, hiy; };

__device__ __forceinline__ EdgeBox edge_box(const double* __restrict__ edges, int e, double pad) {
    const double* r = edges + 5 * (size_t)e;
    const double x0 = r[0], y0 = r[1];
    const double x1 = x0 + r[4] * r[2], y1 = y0 + r[4] * r[3];          // p1 = p0 + len * dir: a multiply, then an add
    EdgeBox b;
    b.lox = (x0 < x1 ? x0 : x1) - pad; b.hix = (x0 > x1 ? x0 : x1) + pad;
    b.loy = (y0 < y1 ? y0 : y1) - pad; b.hiy = (y0 > y1 ? y0 : y1) + pad;
    return b;
}

constexpr int GB = 256;                 // workgroups of the min / max pass (any number gives the same minima and maxima)

__global__ __launch_bounds__(TB) void grid_minmax(const double* __restrict__ edges, int M, double pad, double* __restrict__ part) {
    __shared__ double s[4][TB];
    const int tid = threadIdx.x;
    double m[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
    for (long long e = (long long)blockIdx.x * TB + tid; e < M; e += (long long)gridDim.x * TB) {
        const EdgeBox b = edge_box(edges, (int)e, pad);
        m[0] = b.lox < m[0] ? b.lox : m[0]; m[1] = b.loy < m[1] ? b.loy : m[1];
        m[2] = b.hix > m[2] ? b.hix : m[2]; m[3] = b.hiy > m[3] ? b.hiy : m[3];
    }
    for (int k = 0; k < 4; ++k) s[k][tid] = m[k];
    __syncthreads();
    for (int off = TB / 2; off > 0; off >>= 1) {
        if (tid < off) {
            for (int k = 0; k < 2; ++k) s[k][tid] = s[k][tid + off] < s[k][tid] ? s[k][tid + off] : s[k][tid];
            for (int k = 2; k < 4; ++k) s[k][tid] = s[k][tid + off] > s[k][tid] ? s[k][tid + off] : s[k][tid];
        }
        __syncthreads();
    }
    if (tid == 0) for (int k = 0; k < 4; ++k) part[4 * blockIdx.x + k] = s[k][0];
}

__global__ void grid_origin(const double* __restrict__ part, int nb, double cell, StriveEdgeGridRec* __restrict__ rec) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double m[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
    for (int b = 0; b < nb; ++b) {
        for (int k = 0; k < 2; ++k) m[k] = part[4 * b + k] < m[k] ? part[4 * b + k] : m[k];
        for (int k = 2; k < 4; ++k) m[k] = part[4 * b + k] > m[k] ? part[4 * b + k] : m[k];
    }
    rec->gx0 = floor(m[0]);
    rec->gy0 = floor(m[1]);
    // floor and the division are monotone, so the largest cell index is that of the largest upper bound
    const double nx = floor((m[2] - rec->gx0) / cell) + 1.0, ny = floor((m[3] - rec->gy0) / cell) + 1.0;
    rec->gnx = (nx >= 1.0 && nx < 2147483647.0) ? (int)nx : 0;         // 0: not a finite grid, the host refuses it
    rec->gny = (ny >= 1.0 && ny < 2147483647.0) ? (int)ny : 0;
    rec->total = 0;
}

struct CellRange { int ix0, ix1, iy0, iy1; };
__device__ __forceinline__ CellRange cell_range(const double* __restrict__ edges, int e, double pad, double cell, double gx0, double gy0) {
    const EdgeBox b = edge_box(edges, e, pad);
    CellRange r;
    r.ix0 = (int)floor((b.lox - gx0) / cell); r.ix1 = (int)floor((b.hix - gx0) / cell);
    r.iy0 = (int)floor((b.loy - gy0) / cell); r.iy1 = (int)floor((b.hiy - gy0) / cell);
    return r;
}

__global__ __launch_bounds__(TB) void grid_total(const double* __restrict__ edges, int M, double pad, double cell, StriveEdgeGridRec* __restrict__ rec) {
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= M || rec->gnx == 0 || rec->gny == 0) return;
    const CellRange r = cell_range(edges, e, pad, cell, rec->gx0, rec->gy0);
    atomicAdd((unsigned long long*)&rec->total, (unsigned long long)(r.ix1 - r.ix0 + 1) * (unsigned long long)(r.iy1 - r.iy0 + 1));
}

// pass 0 counts the edges of every cell, pass 1 places them (cursor starts as a copy of cell_ptr)
template <int PASS>
__global__ __launch_bounds__(TB) void grid_place(const double* __restrict__ edges, int M, double pad, double cell, StriveEdgeGridRec rec,
                                                 int* __restrict__ cursor, int* __restrict__ cell_edges, int total) {
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= M) return;
    const CellRange r = cell_range(edges, e, pad, cell, rec.gx0, rec.gy0);
    for (int iy = r.iy0; iy <= r.iy1; ++iy)
        for (int ix = r.ix0; ix <= r.ix1; ++ix) {
            if (ix < 0 || ix >= rec.gnx || iy < 0 || iy >= rec.gny) continue;        // (cannot happen for the record of these edges)
            const int pos = atomicAdd(&cursor[iy * rec.gnx + ix], 1);
            if (PASS == 1 && pos >= 0 && pos < total) cell_edges[pos] = e;
        }
}

// ascending by edge id within a cell: the order in which the atomics of grid_place<1> landed does not survive
__global__ __launch_bounds__(TB) void grid_sort(const int* __restrict__ cell_ptr, int ncell, int* __restrict__ cell_edges) {
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= ncell) return;
    const int a = cell_ptr[c], b = cell_ptr[c + 1];
    for (int i = a + 1; i < b; ++i) {
        const int key = cell_edges[i];
        int j = i - 1;
        while (j >= a && cell_edges[j] > key) {
            cell_edges[j + 1] = cell_edges[j];
            --j;
        }
        cell_edges[j + 1] = key;
    }
}

inline double grid_pad(double margin) { return margin * (1.0 + 1e-9) + 1e-6; }

}  // namespace

extern "C" size_t strive_lane_graph_workspace_bytes(int32_t NL, int32_t P) {
    if (NL < 1 || P < 1) return 0;
    return strive_align_up(lg_work_ints(NL, P) * sizeof(int), 256);
}

static int lg_check_in(const StriveLaneGraphIn* in, const void* ws, size_t ws_bytes) {
    STRIVE_CHECK_ARG(in && ws, "null argument");
    STRIVE_CHECK_ARG(in->NL >= 1 && in->P >= 1, "a map needs at least one lane and one point");
    STRIVE_CHECK_ARG(in->pts && in->lane_ptr && in->out_ptr && in->out_idx && in->in_ptr && in->in_idx, "missing lane tables");
    STRIVE_CHECK_ARG(in->eps >= 0.0, "eps must not be negative");
    STRIVE_CHECK_ARG(ws_bytes >= strive_lane_graph_workspace_bytes(in->NL, in->P), "workspace too small (strive_lane_graph_workspace_bytes)");
    return 0;
}

extern "C" int strive_lane_graph_count(const StriveLaneGraphIn* in, void* ws, size_t ws_bytes, int32_t* counts, strive_stream_t stream) {
    if (lg_check_in(in, ws, ws_bytes) != 0) return -1;
    STRIVE_CHECK_ARG(counts, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const LgWork w = lg_carve(ws, in->NL, in->P);
    const int pb = blocks_for(in->P, TB), lb = blocks_for(in->NL, TB);
    hipLaunchKernelGGL(lg_init, dim3(1), dim3(TB), 0, st, w.first);
    hipLaunchKernelGGL(lg_keep, dim3(pb), dim3(TB), 0, st, *in, w);
    exclusive_scan(w.keep, in->P, w.rank, w.sums, st);
    hipLaunchKernelGGL(lg_trim, dim3(lb), dim3(TB), 0, st, *in, w);
    exclusive_scan(w.lane_n, in->NL, w.node_start, w.sums, st);
    hipLaunchKernelGGL(lg_nodes, dim3(pb), dim3(TB), 0, st, *in, w);
    hipLaunchKernelGGL(lg_degrees, dim3(pb), dim3(TB), 0, st, *in, w);
    exclusive_scan(w.out_deg, in->P, w.succ_ptr, w.sums, st);
    exclusive_scan(w.in_deg, in->P, w.pred_ptr, w.sums, st);
    hipLaunchKernelGGL(lg_counts, dim3(1), dim3(64), 0, st, *in, w, counts);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int strive_lane_graph_fill(const StriveLaneGraphIn* in, void* ws, size_t ws_bytes, const StriveLaneGraphOut* out,
                                      strive_stream_t stream) {
    if (lg_check_in(in, ws, ws_bytes) != 0) return -1;
    STRIVE_CHECK_ARG(out && out->N >= 1 && out->N <= in->P && out->M >= 0 && out->MI >= 0, "bad sizes (take them from strive_lane_graph_count)");
    STRIVE_CHECK_ARG(out->xy && out->succ && out->pred && out->succ_ptr && out->succ_idx && out->succ_len && out->pred_ptr && out->pred_idx &&
                     out->pred_len && out->edges && out->edge_ix, "missing output tables");
    const LgWork w = lg_carve(ws, in->NL, in->P);
    hipLaunchKernelGGL(lg_fill, dim3(blocks_for(out->N, TB)), dim3(TB), 0, (hipStream_t)stream, *in, w, *out);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t strive_edge_grid_workspace_bytes(int32_t M, int64_t ncell) {
    if (M < 1 || ncell < 0) return 0;
    const size_t ints = (size_t)ncell + (size_t)ncell / ST + 2;
    const size_t need = ints * sizeof(int) > GB * 4 * sizeof(double) ? ints * sizeof(int) : GB * 4 * sizeof(double);
    return strive_align_up(need, 256);
}

extern "C" int strive_edge_grid_count(const double* edges, int32_t M, double margin, double cell, void* ws, size_t ws_bytes,
                                      StriveEdgeGridRec* rec, strive_stream_t stream) {
    STRIVE_CHECK_ARG(edges && ws && rec, "null argument");
    STRIVE_CHECK_ARG(M >= 1 && cell > 0.0 && margin >= 0.0, "needs at least one edge, a positive cell and a margin >= 0");
    STRIVE_CHECK_ARG(ws_bytes >= strive_edge_grid_workspace_bytes(M, 0), "workspace too small (strive_edge_grid_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const double pad = grid_pad(margin);
    const int nb = blocks_for(M, TB) < GB ? blocks_for(M, TB) : GB;
    hipLaunchKernelGGL(grid_minmax, dim3(nb), dim3(TB), 0, st, edges, M, pad, (double*)ws);
    hipLaunchKernelGGL(grid_origin, dim3(1), dim3(64), 0, st, (const double*)ws, nb, cell, rec);
    hipLaunchKernelGGL(grid_total, dim3(blocks_for(M, TB)), dim3(TB), 0, st, edges, M, pad, cell, rec);
    STRIVE_CHECK_LAUNCH();
    return 0;
}

extern "C" int strive_edge_grid_fill(const double* edges, int32_t M, double margin, double cell, const StriveEdgeGridRec* rec_host,
                                     void* ws, size_t ws_bytes, int32_t* cell_ptr, int32_t* cell_edges, strive_stream_t stream) {
    STRIVE_CHECK_ARG(edges && ws && rec_host && cell_ptr && cell_edges, "null argument");
    STRIVE_CHECK_ARG(M >= 1 && cell > 0.0 && margin >= 0.0, "needs at least one edge, a positive cell and a margin >= 0");
    const StriveEdgeGridRec rec = *rec_host;
    STRIVE_CHECK_ARG(rec.gnx >= 1 && rec.gny >= 1 && (int64_t)rec.gnx * rec.gny < 0x7fffffffll && rec.total >= 1 && rec.total < 0x7fffffffll,
                     "bad grid record (take it from strive_edge_grid_count)");
    const int ncell = rec.gnx * rec.gny, total = (int)rec.total;
    STRIVE_CHECK_ARG(ws_bytes >= strive_edge_grid_workspace_bytes(M, ncell), "workspace too small (strive_edge_grid_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const double pad = grid_pad(margin);
    int* cursor = (int*)ws;
    int* sums = cursor + ncell;
    const int eb = blocks_for(M, TB);
    hipMemsetAsync(cursor, 0, (size_t)ncell * sizeof(int), st);
    hipLaunchKernelGGL(grid_place<0>, dim3(eb), dim3(TB), 0, st, edges, M, pad, cell, rec, cursor, cell_edges, total);
    exclusive_scan(cursor, ncell, cell_ptr, sums, st);
    hipMemcpyAsync(cursor, cell_ptr, (size_t)ncell * sizeof(int), hipMemcpyDeviceToDevice, st);
    hipLaunchKernelGGL(grid_place<1>, dim3(eb), dim3(TB), 0, st, edges, M, pad, cell, rec, cursor, cell_edges, total);
    hipLaunchKernelGGL(grid_sort, dim3(blocks_for(ncell, TB)), dim3(TB), 0, st, (const int*)cell_ptr, ncell, cell_edges);
    STRIVE_CHECK_LAUNCH();
    return 0;
}
