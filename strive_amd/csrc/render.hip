// Scenario pictures: F (L, L, 3) uint8 RGB pictures of a map crop with cars, trajectories and markers, in one launch.
// (reference src/datasets/nuscenes_utils.py:655-702 viz_map_crop, :717-731 render_map_observation, :733-835
//  render_obj_observation, :837-853 plot_box / plot_car -- one matplotlib figure per picture there)
//
// A pixel (row, col) of a picture stands for the square [col, col + 1] x [L - 1 - row, L - row] of the crop's pixel frame
// (objs2crop's frame: x along the crop's first axis, y along its second, y up; row 0 is the top of the picture).
//
// Background: white, then the map layers in channel order, c += (v_i alpha_i)(col_i - c), v_i the raster byte the crop
// get_map_crop_pos(pose, mapix, bounds, L, L) holds at [i, col, L - 1 - row] -- gathered here through crop_dev.h, the crop itself
// is never written (imshow(x[i].T, origin='lower'), render_map_observation).
//
// Primitives, in table order.  Coverage of a shape on a pixel = (number of the 4 x 4 sub-samples at offsets (k + 1/2)/4 that lie
// in the shape, boundary included) / 16; blend c += (alpha cov)(col - c) in fp32; byte = rint(255 c) clamped.  All inside tests
// are fp32 without fused multiply-adds, so the host emulation of this file computes the same bytes.
//   car      u, v = the sub-sample in the car's frame (heading normalised; a zero heading counts as (1, 0), arctan2(0, 0) = 0).
//            fill     |u| <= l/2 and |v| <= w/2                                                         in the car's colour
//            outline  |u| <= l/2 + e and |v| <= w/2 + e and not (|u| < l/2 - e and |v| < w/2 - e), e = s_edge/2    in black
//            heading  -h <= u <= l/2 + h and |v| <= h, h = s_line/2 (projecting caps)                            in black
//            three blends, each with the car's alpha (plot_box: plt.fill(edgecolor='k') then plt.plot('k')).
//   polyline the union of the capsules of radius s/2 around consecutive vertices, ONE blend (a path is stroked once).
//   disc     distance to the centre <= d/2, one blend per disc.
// A primitive with a NaN in its geometry, and a polyline of fewer than 2 vertices, draws nothing.
//
// Work decomposition: a workgroup of 256 threads owns a 16 x 16 pixel tile of one picture, a thread one pixel.  The picture's
// primitives are walked in passes of 256: thread i of a pass stages primitive i in LDS and tests its bounding box against the
// tile; a ballot per wave turns the 256 verdicts into four 64-bit masks, and every thread then walks the set bits in order -- a
// uniform loop, no compaction, no atomics, no limit on the number of primitives.  The finished tile goes through LDS so that the
// rows leave as aligned 32-bit stores when 3 L is a multiple of 4 (720: yes); otherwise each thread stores its 3 bytes.
#include "common.h"
#include "crop_dev.h"

#pragma clang fp contract(off)

namespace {
constexpr int RT = 16;             // tile edge in pixels
constexpr int RPASS = 256;         // primitives per cull pass = threads per workgroup
constexpr int RPF = STRIVE_RENDER_PRIM_FLOATS;

struct Tile { float x0, y0, x1, y1; };

// conservative: a shape that owns a sub-sample of the tile is never culled (radius grown by 1e-4 relative + 1e-2 pixels against
// the rounding of its own computation); NaN anywhere makes the comparisons false = culled = draws nothing
__device__ __forceinline__ bool box_hits(const Tile& t, float lox, float loy, float hix, float hiy, float grow) {
    const float g = grow * 1.0001f + 0.01f;
    return (hix + g >= t.x0) && (lox - g <= t.x1) && (hiy + g >= t.y0) && (loy - g <= t.y1);
}

__device__ __forceinline__ bool prim_hits_tile(const float* p, const Tile& t, const float* __restrict__ verts, int NV) {
    const int kind = __float_as_int(p[0]);
    if (kind == STRIVE_RENDER_CAR) {
        const float hx = p[3], hy = p[4], l = p[5], w = p[6], se = p[11], sl = p[12];
        if (!(hx == hx) || !(hy == hy) || !(l == l) || !(w == w) || !(se == se) || !(sl == sl)) return false;
        const float a = 0.5f * fabsf(l) + 0.5f * fabsf(se) + 0.5f * fabsf(sl), b = 0.5f * fabsf(w) + 0.5f * fabsf(se) + 0.5f * fabsf(sl);
        return box_hits(t, p[1], p[2], p[1], p[2], sqrtf(a * a + b * b));
    }
    if (kind == STRIVE_RENDER_DISC) return box_hits(t, p[1], p[2], p[1], p[2], 0.5f * p[5]);
    if (kind == STRIVE_RENDER_POLYLINE) {
        const int vb = __float_as_int(p[13]), ve = __float_as_int(p[14]);
        if (vb < 0 || ve > NV || ve - vb < 2) return false;
        float lox = verts[2 * vb], hix = lox, loy = verts[2 * vb + 1], hiy = loy;
        bool ok = (lox == lox) && (loy == loy);
        for (int i = vb + 1; i < ve; ++i) {
            const float x = verts[2 * i], y = verts[2 * i + 1];
            ok = ok && (x == x) && (y == y);
            lox = fminf(lox, x); hix = fmaxf(hix, x);
            loy = fminf(loy, y); hiy = fmaxf(hiy, y);
        }
        return ok && box_hits(t, lox, loy, hix, hiy, 0.5f * p[11]);
    }
    return false;
}

__device__ __forceinline__ void blend(float c[3], float r, float g, float b, float alpha, int count) {
    if (count == 0) return;
    const float a = alpha * ((float)count * 0.0625f);
    c[0] = c[0] + a * (r - c[0]);
    c[1] = c[1] + a * (g - c[1]);
    c[2] = c[2] + a * (b - c[2]);
}

// the pixel whose lower-left corner is (fx, fy): sub-sample (k, j) sits at (fx + (k + 1/2)/4, fy + (j + 1/2)/4)
__device__ __forceinline__ void draw_prim(const float* p, float fx, float fy, const float* __restrict__ verts, float c[3]) {
    const int kind = __float_as_int(p[0]);
    if (kind == STRIVE_RENDER_CAR) {
        const float cx = p[1], cy = p[2], hx = p[3], hy = p[4];
        const float n = sqrtf(hx * hx + hy * hy);
        const float ux = n > 0.0f ? hx / n : 1.0f, uy = n > 0.0f ? hy / n : 0.0f;
        const float hl = 0.5f * p[5], hw = 0.5f * p[6], he = 0.5f * p[11], hs = 0.5f * p[12];
        int nf = 0, ne = 0, nh = 0;
        for (int j = 0; j < 4; ++j) {
            const float dy = (fy + ((float)j + 0.5f) * 0.25f) - cy;
            for (int k = 0; k < 4; ++k) {
                const float dx = (fx + ((float)k + 0.5f) * 0.25f) - cx;
                const float u = dx * ux + dy * uy, v = dy * ux - dx * uy;
                const float au = fabsf(u), av = fabsf(v);
                nf += (au <= hl && av <= hw) ? 1 : 0;
                ne += (au <= hl + he && av <= hw + he && !(au < hl - he && av < hw - he)) ? 1 : 0;
                nh += (u >= -hs && u <= hl + hs && av <= hs) ? 1 : 0;
            }
        }
        blend(c, p[7], p[8], p[9], p[10], nf);
        blend(c, 0.0f, 0.0f, 0.0f, p[10], ne);
        blend(c, 0.0f, 0.0f, 0.0f, p[10], nh);
    } else if (kind == STRIVE_RENDER_DISC) {
        const float cx = p[1], cy = p[2], r = 0.5f * p[5], r2 = r * r;
        int nd = 0;
        for (int j = 0; j < 4; ++j) {
            const float dy = (fy + ((float)j + 0.5f) * 0.25f) - cy;
            for (int k = 0; k < 4; ++k) {
                const float dx = (fx + ((float)k + 0.5f) * 0.25f) - cx;
                nd += (r >= 0.0f && dx * dx + dy * dy <= r2) ? 1 : 0;
            }
        }
        blend(c, p[7], p[8], p[9], p[10], nd);
    } else {
        const int vb = __float_as_int(p[13]), ve = __float_as_int(p[14]);
        const float r = 0.5f * p[11], r2 = r * r;
        unsigned in = 0;                                   // bit 4 j + k: the sub-sample lies in some capsule
        float ax = verts[2 * vb], ay = verts[2 * vb + 1];
        for (int i = vb + 1; i < ve && in != 0xffffu; ++i) {
            const float bx = verts[2 * i], by = verts[2 * i + 1];
            const float ex = bx - ax, ey = by - ay, len2 = ex * ex + ey * ey;
            for (int j = 0; j < 4; ++j) {
                const float qy = (fy + ((float)j + 0.5f) * 0.25f) - ay;
                for (int k = 0; k < 4; ++k) {
                    const float qx = (fx + ((float)k + 0.5f) * 0.25f) - ax;
                    float t = len2 > 0.0f ? (qx * ex + qy * ey) / len2 : 0.0f;
                    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
                    const float dx = qx - t * ex, dy = qy - t * ey;
                    if (r >= 0.0f && dx * dx + dy * dy <= r2) in |= 1u << (4 * j + k);
                }
            }
            ax = bx; ay = by;
        }
        blend(c, p[7], p[8], p[9], p[10], __builtin_popcount(in));
    }
}

__global__ __launch_bounds__(RPASS) void render_kernel(StriveMap map, StriveRenderJob job, uint8_t* __restrict__ out, int dword_rows) {
    __shared__ float s_prim[RPASS * RPF];
    __shared__ unsigned long long s_mask[RPASS / 64];
    __shared__ uint32_t s_out[RT * RT * 3 / 4];
    const int L = job.L, f = blockIdx.y, tid = threadIdx.x;
    const int tiles_x = (L + RT - 1) / RT;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int row = ty * RT + (tid >> 4), col = tx * RT + (tid & 15);
    const bool live = row < L && col < L;
    float c[3] = {1.0f, 1.0f, 1.0f};

    // ---- background: the map layers at crop index [i, col, L - 1 - row] ----
    const int m = job.mapix[f];
    if (live && !job.no_map[f] && m >= 0 && m < map.M) {
        CropFrame fr;
        fr.x = job.pose[f * 4 + 0]; fr.y = job.pose[f * 4 + 1]; fr.hc = job.pose[f * 4 + 2]; fr.hs = job.pose[f * 4 + 3];
        set_crop_scale(fr, map.dx[m * 2 + 0], map.dx[m * 2 + 1]);
        fr.H = map.H; fr.W = map.W;
        fr.base = map.raster + (size_t)m * map.C * map.H * map.W;
        const float* lin = job.lin + (size_t)job.lin_ix[f] * 2 * L;
        int px, py;
        crop_pixel(fr, lin[col], lin[L + (L - 1 - row)], true, px, py);
        const uint8_t* src = fr.base + (size_t)py * map.W + px;
        const size_t plane = (size_t)map.H * map.W;
        for (int i = 0; i < map.C; ++i) {
            const float a = (float)src[i * plane] * job.layer_alpha[i];
            for (int k = 0; k < 3; ++k) c[k] = c[k] + a * (job.layer_rgb[i * 3 + k] - c[k]);
        }
    }

    // ---- primitives, in passes of RPASS ----
    int p0 = job.prim_range[f * 2 + 0], p1 = job.prim_range[f * 2 + 1];
    p0 = p0 < 0 ? 0 : p0;
    p1 = p1 > job.NP ? job.NP : p1;
    Tile t;
    t.x0 = (float)(tx * RT); t.x1 = (float)(tx * RT + RT);
    t.y1 = (float)(L - ty * RT); t.y0 = (float)(L - ty * RT - RT);
    const float fx = (float)col, fy = (float)(L - 1 - row);
    for (int base = p0; base < p1; base += RPASS) {
        __syncthreads();
        bool keep = false;
        if (base + tid < p1) {
            const float4* src = reinterpret_cast<const float4*>(job.prims + (size_t)(base + tid) * RPF);
            float4* dst = reinterpret_cast<float4*>(s_prim + tid * RPF);
            for (int q = 0; q < RPF / 4; ++q) dst[q] = src[q];
            keep = prim_hits_tile(s_prim + tid * RPF, t, job.verts, job.NV);
        }
        const unsigned long long bal = __ballot(keep ? 1 : 0);
        if ((tid & 63) == 0) s_mask[tid >> 6] = bal;
        __syncthreads();
        for (int wv = 0; wv < RPASS / 64; ++wv) {
            unsigned long long msk = s_mask[wv];
            while (msk) {
                const int b = __ffsll((long long)msk) - 1;
                msk &= msk - 1;
                if (live) draw_prim(s_prim + (wv * 64 + b) * RPF, fx, fy, job.verts, c);
            }
        }
    }

    // ---- bytes ----
    uint8_t rgb[3];
    for (int k = 0; k < 3; ++k) {
        float v = rintf(255.0f * c[k]);
        v = v >= 0.0f ? v : 0.0f;                  // NaN -> 0
        rgb[k] = (uint8_t)(v > 255.0f ? 255.0f : v);
    }
    if (!dword_rows) {
        if (live) {
            uint8_t* o = out + ((size_t)((size_t)f * L + row) * L + col) * 3;
            o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
        }
        return;
    }
    uint8_t* s_b = reinterpret_cast<uint8_t*>(s_out);
    for (int k = 0; k < 3; ++k) s_b[tid * 3 + k] = rgb[k];
    __syncthreads();
    if (tid < RT * 12) {
        // L is a multiple of 4 and the tile starts at a multiple of 16 pixels: its live part of a row is a whole number of words
        const int r = tid / 12, d = tid - r * 12;
        const int orow = ty * RT + r;
        const int live_words = ((L - tx * RT < RT ? L - tx * RT : RT) * 3) / 4;
        if (orow < L && d < live_words)
            reinterpret_cast<uint32_t*>(out + ((size_t)((size_t)f * L + orow) * L + tx * RT) * 3)[d] = s_out[r * 12 + d];
    }
}
}  // namespace

extern "C" int strive_render_pictures(const StriveMap* map, const StriveRenderJob* job, uint8_t* out, strive_stream_t stream) {
    STRIVE_CHECK_ARG(map && job && out, "null argument");
    STRIVE_CHECK_ARG(job->F >= 0 && job->L > 0 && job->NP >= 0 && job->NV >= 0, "bad sizes");
    STRIVE_CHECK_ARG(job->W == job->L, "only square pictures (L == W) are rendered");
    STRIVE_CHECK_ARG(map->C >= 1 && map->C <= STRIVE_RENDER_MAX_LAYERS, "the map has more layers than the colour list (6)");
    STRIVE_CHECK_ARG(job->L <= 16384 && job->F <= 65535, "picture too large or too many pictures for one launch");
    if (job->F == 0) return 0;
    STRIVE_CHECK_ARG(job->pose && job->mapix && job->lin && job->lin_ix && job->prim_range && job->no_map, "missing per-picture tables");
    STRIVE_CHECK_ARG((job->NP == 0 || job->prims) && (job->NV == 0 || job->verts), "missing primitive tables");
    STRIVE_CHECK_ARG((((uintptr_t)job->prims) & 15) == 0, "the primitive table must be 16-byte aligned");
    const int tiles = (job->L + RT - 1) / RT;
    const int dword_rows = (job->L % 4 == 0) && ((((uintptr_t)out) & 3) == 0);
    hipLaunchKernelGGL(render_kernel, dim3(tiles * tiles, job->F), dim3(RPASS), 0, (hipStream_t)stream, *map, *job, out, dword_rows);
    STRIVE_CHECK_LAUNCH();
    return 0;
}
