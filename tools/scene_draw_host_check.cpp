// Stand-alone host run of strive_scene_draw_tables for sanitizers: links the host-emulation build of strive_amd/csrc/scene_draw.hip
// (tests/hipemu) and draws a ragged batch of five scenes (257 + 1 + 17 + 2 + 65 agents, NaN lead-ins, gaps and tails) with every
// kind of view.  Every table is allocated at its exact size, so a store past a slot is a heap overflow the sanitizer reports.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   $CXX -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -I tests/hipemu \
//        tools/scene_draw_host_check.cpp strive_amd/csrc/scene_draw.hip strive_amd/csrc/capi.hip tests/hipemu/hipemu.cpp -o scene_draw_host_check
//   ASAN_OPTIONS=detect_leaks=0 ./scene_draw_host_check          (host only: never on a GPU machine, never through Python)
// (the emulator keeps its 256 fiber stacks for the life of the process, tests/hipemu/hipemu.cpp; the leak check would report those)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/strive_hip.h"

static unsigned long long g_state = 88172645463325252ull;
static float uniform(float lo, float hi) {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return lo + (hi - lo) * (float)((g_state >> 11) & 0xffffff) / 16777216.0f;
}

int main() {
    const int sizes[5] = {257, 1, 17, 2, 65}, B = 5, PT = 4, FT = 12, NS = 3, FPT = 5, L = 32;
    std::vector<int32_t> ptr(B + 1, 0);
    for (int b = 0; b < B; ++b) ptr[b + 1] = ptr[b] + sizes[b];
    const int NA = ptr[B];
    const float nan = std::nanf("");
    std::vector<float> past((size_t)NA * PT * 6), fut((size_t)NA * FT * 6), lw((size_t)NA * 2), pred((size_t)NA * NS * FPT * 4), ow((size_t)NA * FT * 4);
    for (auto* v : {&past, &fut, &lw, &pred, &ow}) for (float& x : *v) x = uniform(-1.5f, 1.5f);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < sizes[b]; ++j) {
            const int a = ptr[b] + j;
            if (j % 7 == 1) for (int c = 0; c < 12; ++c) past[(size_t)a * PT * 6 + c] = nan;                        // lead-in
            if (j % 7 == 2) for (int c = 0; c < 12; ++c) fut[((size_t)a * FT + 4) * 6 + c] = nan;                    // gap
            if (j % 7 == 3) for (int t = 8; t < FT; ++t) fut[((size_t)a * FT + t) * 6] = nan;                       // tail
            if (j % 7 == 4) { for (int c = 0; c < PT * 6; ++c) past[(size_t)a * PT * 6 + c] = nan; for (int c = 0; c < FT * 6; ++c) fut[(size_t)a * FT * 6 + c] = nan; }
            if (j % 7 == 5) pred[((size_t)a * NS + 1) * FPT * 4 + 8] = nan;
        }
    std::vector<int64_t> map_idx = {0, 1, 0, 1, 0};
    // views: per scene an overview with trajectories over the ground truth, cars around the centroid, one agent at crop_t with
    // ow_gt; a video of the scene (cars), and for the clean two-agent scene a video with trajectories
    std::vector<int32_t> views, pics, nomap;
    std::vector<float> view_f, style;
    int NP = 0, NV = 0;
    const int NT = PT + FPT, gNT = PT + FT;
    const int rb_pred = 0, rb_gt = NT, rb_one = NT + gNT, rb_rows = NT + gNT + 1;
    auto view = [&](int b, int flags, int d0, int dn, int g0, int gn, int crop_t, int set, int sty) {
        const int32_t rec[STRIVE_SCENE_DRAW_VIEW_INTS] = {b, flags, d0, dn, g0, gn, crop_t, set, rb_pred, sty};
        views.insert(views.end(), rec, rec + STRIVE_SCENE_DRAW_VIEW_INTS);
        const float f[4] = {-45.0f, -45.0f, (float)(L / 90.0), (float)(L / 90.0)};
        view_f.insert(view_f.end(), f, f + 4);
        return (int)(views.size() / STRIVE_SCENE_DRAW_VIEW_INTS) - 1;
    };
    auto picture = [&](int v, int s, int t, int dn, int gn, int ns, int nt, bool traj) {
        const int steps = gn * gNT + dn * ns * nt;
        const int pcap = traj ? steps + gn + dn * ns + dn : steps, vcap = traj ? steps : 0;
        const int32_t rec[STRIVE_SCENE_DRAW_PIC_INTS] = {v, s, t, NP, NV, pcap, vcap, 0};
        pics.insert(pics.end(), rec, rec + STRIVE_SCENE_DRAW_PIC_INTS);
        NP += pcap; NV += vcap;
    };
    for (int b = 0; b < B; ++b) {
        const int n = sizes[b];
        const int sty = (int)(style.size() / 8);
        for (int j = 0; j < n; ++j) for (int c = 0; c < 8; ++c) style.push_back(c < 4 ? 0.5f : 2.0f);
        picture(view(b, STRIVE_SCENE_DRAW_TRAJ, 0, n, 0, n, 0, 0, -1), -1, 0, n, n, NS, NT, true);
        picture(view(b, STRIVE_SCENE_DRAW_CENTER, 0, n, 0, n, 0, 0, sty), -1, 0, n, n, NS, NT, false);
        picture(view(b, STRIVE_SCENE_DRAW_TRAJ | STRIVE_SCENE_DRAW_CROP_T | STRIVE_SCENE_DRAW_OW_GT, n - 1, 1, n - 1, 1, 9, 0, sty), -1, 0, 1, 1, NS, NT, true);
        picture(view(b, STRIVE_SCENE_DRAW_TRAJ | STRIVE_SCENE_DRAW_CENTER, 0, n, 0, 0, 0, -1, -1), -1, 0, n, 0, 1, gNT, true);
        const int v = view(b, STRIVE_SCENE_DRAW_CENTER, 0, n, 0, 0, 0, 0, sty);
        for (int s = 0; s < NS; ++s) for (int t = 0; t < NT; ++t) picture(v, s, t, n, 0, 1, 1, false);
        if (b == 3) {
            const int w = view(b, STRIVE_SCENE_DRAW_TRAJ, 0, n, 0, 0, 0, 0, -1);
            for (int s = 0; s < NS; ++s) for (int t = 0; t < NT; ++t) picture(w, s, t, n, 0, 1, 1, true);
        }
    }
    // records that do not fit: the kernel must refuse them without touching memory
    picture(view(0, 0, 250, 20, 0, 0, 0, 0, -1), -1, 0, 20, 0, NS, NT, false);
    picture(view(9, 0, 0, 1, 0, 0, 0, 0, -1), -1, 0, 1, 0, NS, NT, false);
    picture(view(1, 0, 0, 1, 0, 0, 0, 3, -1), -1, 0, 1, 0, NS, NT, false);
    const int F = (int)(pics.size() / STRIVE_SCENE_DRAW_PIC_INTS), NVIEW = (int)(views.size() / STRIVE_SCENE_DRAW_VIEW_INTS);
    std::vector<float> rainbow((size_t)rb_rows * 3, 0.25f);
    // outputs at their exact sizes; prims 16-byte aligned by operator new's alignment for a float4-sized type
    float* prims = static_cast<float*>(operator new((size_t)NP * 16 * sizeof(float), std::align_val_t(16)));
    std::vector<float> verts((size_t)NV * 2), pose((size_t)F * 4);
    std::vector<int32_t> mapix(F), range((size_t)F * 2), status(F);
    StriveSceneDraw job = {};
    job.past_gt = past.data(); job.future_gt = fut.data(); job.lw = lw.data(); job.ow_gt = ow.data(); job.pred[0] = pred.data();
    job.pred_NS[0] = NS; job.pred_FPT[0] = FPT;
    job.scene_ptr = ptr.data(); job.map_idx = map_idx.data(); job.views = views.data(); job.view_f = view_f.data(); job.pictures = pics.data();
    job.style = style.data(); job.rainbow = rainbow.data();
    job.pose = pose.data(); job.mapix = mapix.data(); job.prim_range = range.data(); job.prims = prims; job.verts = verts.data(); job.status = status.data();
    job.k = 0.1; job.NA = NA; job.B = B; job.M = 2; job.PT = PT; job.FT = FT; job.past_stride = 6; job.future_stride = 6;
    job.NVIEW = NVIEW; job.F = F; job.NP = NP; job.NV = NV;
    job.rb_rows = rb_rows; job.rb_gt_off = rb_gt; job.rb_one_off = rb_one; job.style_rows = (int)(style.size() / 8);
    job.edge_px = 0.1f; job.heading_px = 0.15f;
    for (int i = 0; i < 6; ++i) { job.norm.state_mean[i] = 100.0f; job.norm.state_std[i] = 20.0f; }
    for (int i = 0; i < 2; ++i) { job.norm.att_mean[i] = 4.0f; job.norm.att_std[i] = 1.0f; }
    const int rc = strive_scene_draw_tables(&job, nullptr);
    if (rc != 0) { fprintf(stderr, "strive_scene_draw_tables failed: %s\n", strive_last_error()); return 1; }
    long long drawn = 0;
    int refused = 0, nostep = 0;
    for (int f = 0; f < F; ++f) {
        const int n = range[2 * f + 1] - range[2 * f];
        if (n < 0 || n > pics[(size_t)f * STRIVE_SCENE_DRAW_PIC_INTS + 5]) { fprintf(stderr, "picture %d: %d records in a slot of %d\n", f, n, pics[(size_t)f * 8 + 5]); return 1; }
        drawn += n;
        refused += (status[f] & STRIVE_SCENE_DRAW_BAD_VIEW) != 0;
        nostep += (status[f] & STRIVE_SCENE_DRAW_NO_STEP) != 0;
    }
    printf("%d pictures of %d views, %lld records in %d slots, %d vertex slots; %d refused records, %d pictures with an unobserved agent\n", F, NVIEW,
           drawn, NP, NV, refused, nostep);
    operator delete(prims, std::align_val_t(16));
    return refused == 3 ? 0 : 1;
}
