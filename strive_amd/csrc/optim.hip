// The optimiser step of the training loop (reference src/train_traffic.py:113-115, :275-277: optim.Adam over model.parameters()):
// ONE launch over the flat parameter / gradient / moment buffers, which also leaves max |w| of every parameter tensor on the device
// (the weight packs that follow every update need it: params.py).  The step is launch-latency-bound (1.09 M parameters, ~35 MB of
// traffic), so the kernel is plain: one 16-byte vector of each array per thread, a binary search in the segment table per thread,
// one atomic per wave wherever a wave lies inside one tensor.
#include "common.h"

#include <math.h>

namespace {

struct AdamArgs {
    float w1;          // 1 - beta1 (lerp weight of exp_avg)
    float beta1;       // lerp's other branch (weight >= 0.5) multiplies by 1 - weight
    float beta2, w2;   // w2 = 1 - beta2
    float step;        // lr / bc1
    float sqrt_bc2;
    float eps, wd;
};

// torch.optim.Adam, single-tensor form (torch/optim/adam.py _single_tensor_adam), one element:
//   grad = grad.add(param, alpha=wd);  exp_avg.lerp_(grad, 1 - beta1);  exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//   denom = (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps);  param.addcdiv_(exp_avg, denom, value=-lr / bc1)
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamArgs& a) {
    if (a.wd != 0.f) g = g + a.wd * p;
    const float d = g - m;
    m = a.w1 < 0.5f ? m + a.w1 * d : g - d * a.beta1;
    v = v * a.beta2 + (a.w2 * g) * g;
    const float denom = sqrtf(v) / a.sqrt_bc2 + a.eps;
    p = p - a.step * (m / denom);
}

// the tensor that holds element i: the s in [0, nseg) with seg_off[s] <= i < seg_off[s + 1] (empty tensors are passed over)
__device__ __forceinline__ int segment_of(const int64_t* __restrict__ seg_off, int nseg, int64_t i) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// max |p| per tensor as an unsigned maximum of the bit patterns of |p|: for non-negative floats the integer order is the float
// order, every NaN pattern lies above infinity (a NaN wins and stays a NaN), and an integer maximum does not depend on the order.
static __global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                 float* __restrict__ v, int64_t n, AdamArgs a,
                                                                 const int64_t* __restrict__ seg_off, int nseg,
                                                                 unsigned* __restrict__ seg_absmax) {
    const int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    float np[4] = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    if (base + 4 <= n) {
        const float4 p4 = *reinterpret_cast<const float4*>(p + base), g4 = *reinterpret_cast<const float4*>(g + base);
        float4 m4 = *reinterpret_cast<const float4*>(m + base), v4 = *reinterpret_cast<const float4*>(v + base);
        np[0] = p4.x; np[1] = p4.y; np[2] = p4.z; np[3] = p4.w;
        adam_element(np[0], g4.x, m4.x, v4.x, a);
        adam_element(np[1], g4.y, m4.y, v4.y, a);
        adam_element(np[2], g4.z, m4.z, v4.z, a);
        adam_element(np[3], g4.w, m4.w, v4.w, a);
        *reinterpret_cast<float4*>(p + base) = make_float4(np[0], np[1], np[2], np[3]);
        *reinterpret_cast<float4*>(m + base) = m4;
        *reinterpret_cast<float4*>(v + base) = v4;
        cnt = 4;
    } else if (base < n) {                                   // the last, partial vector
        cnt = (int)(n - base);
        for (int j = 0; j < cnt; ++j) {
            float mj = m[base + j], vj = v[base + j];
            np[j] = p[base + j];
            adam_element(np[j], g[base + j], mj, vj, a);
            p[base + j] = np[j];
            m[base + j] = mj;
            v[base + j] = vj;
        }
    }
    if (seg_absmax == nullptr) return;
    // every lane stays for the wave exchange: a lane past the end stands on the last element and contributes nothing
    const int64_t first = base < n ? base : n - 1;
    const int64_t last = base + 3 < n ? base + 3 : n - 1;
    const int s_first = segment_of(seg_off, nseg, first);
    int s_last = s_first;
    while (s_last < nseg - 1 && seg_off[s_last + 1] <= last) ++s_last;
    const int w_first = __shfl(s_first, 0), w_last = __shfl(s_last, 63);
    if (w_first == w_last) {                                 // the wave lies inside one tensor: one atomic
        unsigned mx = 0;
        for (int j = 0; j < cnt; ++j) {
            const unsigned b = abs_bits(np[j]);
            mx = b > mx ? b : mx;
        }
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_xor(mx, d);
            mx = o > mx ? o : mx;
        }
        if ((threadIdx.x & 63) == 0 && mx != 0) atomicMax(seg_absmax + w_first, mx);
        return;
    }
    int s = s_first;
    unsigned mx = 0;
    for (int j = 0; j < cnt; ++j) {
        while (s < nseg - 1 && seg_off[s + 1] <= base + j) {
            if (mx != 0) atomicMax(seg_absmax + s, mx);
            mx = 0;
            ++s;
        }
        const unsigned b = abs_bits(np[j]);
        mx = b > mx ? b : mx;
    }
    if (mx != 0) atomicMax(seg_absmax + s, mx);
}

}  // namespace

extern "C" int strive_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                                double weight_decay, double bc1, double bc2, const int64_t* seg_off, int32_t nseg, float* seg_absmax,
                                strive_stream_t stream) {
    STRIVE_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 40), "bad element count");
    STRIVE_CHECK_ARG(seg_absmax == nullptr || (seg_off != nullptr && nseg > 0), "seg_absmax needs a segment table");
    if (n > 0) {                                   // every argument is checked before anything is written
        STRIVE_CHECK_ARG(p && g && m && v, "NULL array");
        STRIVE_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "the flat arrays must be 16-byte aligned");
        STRIVE_CHECK_ARG(bc1 > 0.0 && bc2 > 0.0, "bias corrections must be positive (step count >= 1)");
    }
    if (seg_absmax != nullptr && hipMemsetAsync(seg_absmax, 0, (size_t)nseg * sizeof(float), (hipStream_t)stream) != hipSuccess) {
        strive_set_error("%s: clearing the max |w| table failed", __func__);
        return -2;
    }
    if (n == 0) return 0;
    AdamArgs a;
    a.w1 = (float)(1.0 - beta1);
    a.beta1 = (float)beta1;
    a.beta2 = (float)beta2;
    a.w2 = (float)(1.0 - beta2);
    a.step = (float)(lr / bc1);
    a.sqrt_bc2 = (float)sqrt(bc2);
    a.eps = (float)eps;
    a.wd = (float)weight_decay;
    const int64_t vecs = (n + 3) / 4;
    hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, a, seg_off,
                       (int)nseg, (unsigned*)seg_absmax);
    STRIVE_CHECK_LAUNCH();
    return 0;
}
