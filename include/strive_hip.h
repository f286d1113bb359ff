/* strive_hip.h -- C ABI of libstrive_hip.so: STRIVE's latent-optimisation hot path on MI355X (gfx950).
 *
 * The reference (nv-tlabs/STRIVE) is pure Python/PyTorch and has no FFI; its boundary for this path is
 * the Python surface of src/models/traffic_model.py, src/models/interaction_net.py,
 * src/datasets/nuscenes_utils.py and src/losses/adv_gen_nusc.py.  Each entry point below names the
 * reference function (file:line under /root/reference) whose arithmetic it replaces; INTEGRATION.md
 * shows the ctypes stub a maintainer of the reference would add at those lines.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless the comment says "host";
 *   - fp32 tensors are row-major contiguous; index tensors are int32; the raster is uint8, metres-per-
 *     pixel is float64 (as the reference keeps it, src/datasets/map_env.py:166);
 *   - nothing is allocated or freed: the caller passes outputs and a workspace whose size comes from the
 *     matching *_bytes() query; workspaces are scratch (contents undefined on return) except "tape";
 *   - work is enqueued on `stream` (a hipStream_t passed as void*), no hidden synchronisation;
 *   - return 0 on success, a negative code on failure; strive_last_error() (thread local) explains it;
 *   - re-entrant; no global mutable state besides the error string and the options below.  One exception (round 5): strive_rollout_bwd_train_kept forks
 *     the map CNN's backward onto a library-owned side stream (one per device, created at first use) and joins it back on `stream`
 *     with events before it returns -- no host synchronisation, the caller's stream order is what it would be without it; one
 *     such call at a time per device: a second host thread entering while the first is still enqueueing gets -3 (ABI 17; it was
 *     a documented rule only), and a device on which the stream or its events cannot be created runs without the overlap.
 */
#ifndef STRIVE_HIP_H
#define STRIVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STRIVE_ABI_VERSION 17
#define STRIVE_HID 128        /* hidden width of every MLP in the reference (models/common.py, interaction_net.py:32,41) */
#define STRIVE_MAX_LAYERS 4
/* Latent width Z of the shipped model (latent_size=32).  The library takes a decoder's Z from its pack:
 * Z = gnn.mlp_in.dims[0] - (64 + 64 + NC + 2), any width from 1 to 64; every z / dz buffer of the rollout entry points has
 * row stride Z. */
#define STRIVE_ZDIM 32
#define STRIVE_FEAT 64        /* map / past feature size and GRU hidden size (traffic_model.py:25-27) */

typedef void* strive_stream_t;

int strive_abi_version(void);
const char* strive_last_error(void);

/* Options (ABI 17).  Up to round 5 the library read 19 undeclared environment variables inside its entry points; it reads none
 * any more.  Every switch is a named process-wide integer with the shipped behaviour as its default; a caller that never touches
 * them gets exactly the documented behaviour.  Set them between calls (a call reads them when it starts); they are plain ints, not
 * synchronised against calls running on other threads.  Reference: none (the reference has no native side to tune); the Python host
 * (strive_amd/_lib.py) maps an environment variable STRIVE_<NAME> onto option <name> when the library is loaded and on
 * sync_options_from_env().
 *   algorithm choices (results agree to rounding, mostly bit for bit -- the A/B switches of DESIGN.md section 4):
 *     cnn_small_batch (96)   map CNN: a launch of <= this many samples runs the small-batch kernel forms (0: never)
 *     cnn_chunk (512)        samples pushed through the CNN layer stack together (8 .. 1024)
 *     cnn_tail_s (0)         samples per workgroup of the fused CNN tail: 0 = by size, or 1 / 2 / 4
 *     conv_ws (1)            conv2 on specialised producer / consumer waves (0: conv_bf6_kernel; bit-identical)
 *     conv_wsx (1)           conv3 / conv4 on specialised waves with streamed weights (0: conv_bf6_kernel; bit-identical)
 *     scene_kernels (1)      scene-resident decoder kernels where they apply (0: launch-per-phase kernels)
 *     scene_tiles (1)        batches with scenes of > 16 agents: the forward step's node-level phases on the scene kernel in 16-row
 *                            tiles (0: launch-per-phase kernels; results agree to fp32 rounding)
 *     scene_split (12)       scenes of >= this many agents share their edge chunks among K workgroups (0: never)
 *     scene_fwd_k (-1)       K of the forward step (-1: one workgroup per 64-row edge chunk, <= 4)
 *     sweep_step (-1)        reverse sweep as one launch per step on K workgroups per scene (-1: from 3 chunks on; 0: never; 1..4)
 *     train_overlap (1)      strive_rollout_bwd_train_kept: CNN backward of finished steps on the library's side stream
 *     train_overlap_rows (256)  samples per hand-over to that stream
 *     wgrad_atomics, dgrad_igemm, wgrad_igemm, wgrad_tile (0)   earlier forms of the training backward kept for A/B
 *   measurement hooks (results of the affected call are INVALID or the workspace tail is written; never set in production):
 *     conv_ws_dbg (bit mask), wgrad_dbg, scene_prof, planner_prof, planner_dbg (bit mask)
 * strive_set_option / strive_get_option return 0, or -1 for an unknown name or a value outside the option's range
 * (strive_last_error() names it); strive_option_name(i), 0 <= i < strive_option_count(), enumerates the names. */
int strive_set_option(const char* name_host, int64_t value);
int strive_get_option(const char* name_host, int64_t* value_host);
int strive_reset_options(void);
int32_t strive_option_count(void);
const char* strive_option_name(int32_t i);

/* ------------------------------------------------------------------------------------------------
 * Shared descriptors (host structs holding device pointers)
 * ---------------------------------------------------------------------------------------------- */

/* Linear -> (LayerNorm -> ReLU -> Linear)* ; reference src/models/common.py:8-44.
 * w[l]  : torch layout (dims[l+1], dims[l])      -- used by the backward (input-gradient) kernels
 * wt[l] : transposed   (dims[l],   dims[l+1])    -- used by the forward kernels
 * ln_g/ln_b[l] : LayerNorm(dims[l+1]) applied to the output of layer l, l < nlayers-1 (eps 1e-5). */
typedef struct StriveMLP {
    int32_t nlayers;
    int32_t dims[STRIVE_MAX_LAYERS + 1];
    const float* w[STRIVE_MAX_LAYERS];
    const float* wt[STRIVE_MAX_LAYERS];
    const float* b[STRIVE_MAX_LAYERS];
    const float* ln_g[STRIVE_MAX_LAYERS];
    const float* ln_b[STRIVE_MAX_LAYERS];
    /* optional (NULL = the layer runs on the vector ALUs from w / wt): W_l * wsc[l] (wf) and its transpose (wbf) split into two
     * fp16 pieces (w0 = fp16(w) to nearest, w1 = fp16(w - w0)) in the operand order of v_mfma_f32_16x16x32_f16:
     * [row tile = row / 16][k-step = k / 32][piece][lane 0..63][8 x fp16], lane l = row 16 tile + (l & 15),
     * k = 32 step + 8 (l >> 4) + j, zero beyond the matrix; rows = outputs and k = inputs for wf, the reverse for wbf.
     * wsc[l] is a power of two. */
    const void* wf[STRIVE_MAX_LAYERS];
    const void* wbf[STRIVE_MAX_LAYERS];
    float wsc[STRIVE_MAX_LAYERS];
} StriveMLP;

/* One message-passing round over per-scene cliques; reference src/models/interaction_net.py:16-218
 * (k=1, MLP update, max aggregation).  edge.dims[0] = 2*(D+NC)+4, update.dims[0] = 2*D+NC. */
typedef struct StriveGNN {
    StriveMLP mlp_in, edge, update, mlp_out;
    int32_t D;   /* node embedding size during message passing: 64 (decoder) or 128 (prior/posterior) */
    int32_t NC;  /* semantic classes */
} StriveGNN;

/* 3-layer GRU memory, hidden 64, input 4; reference src/models/traffic_model.py:151-156.
 * wih_t[l]: (in_l, 192) with in_0 = 4, in_1 = in_2 = 64;  whh_t[l]: (64, 192); gate order r,z,n.
 * wih[l], whh[l]: torch layouts (192, in_l), (192, 64) for the backward kernels.
 * Optional matrix-core operands (ABI 14; NULL = the scene-resident rollout kernels are not used): whh_f[l] / wih_f[l] = the
 * two-piece fp16 fragments (StriveMLP.wf layout) of whh[l] * hh_sc[l] / wih[l] * ih_sc[l] (rows = the 192 gate outputs),
 * whh_bf[l] / wih_bf[l] those of the transposes (rows = the 64 inputs: the input-gradient products of the reverse sweep).
 * Layer 0's input is 4 wide: wih_f[0] / wih_bf[0] stay NULL (that product runs on the vector ALUs). */
typedef struct StriveGRU {
    const float* wih[3];
    const float* whh[3];
    const float* wih_t[3];
    const float* whh_t[3];
    const float* bih[3];
    const float* bhh[3];
    const void* whh_f[3];
    const void* wih_f[3];
    const void* whh_bf[3];
    const void* wih_bf[3];
    float hh_sc[3];
    float ih_sc[3];
} StriveGRU;

/* Rasterised maps + crop geometry; reference src/datasets/map_env.py:50-61,165-166 and
 * src/datasets/nuscenes_utils.py:205-232.  lwise/wwise are the fp32 linspace tables over the crop
 * bounds ([-17,60] m along the heading, [-38.5,38.5] m across), computed by the caller. */
typedef struct StriveMap {
    const uint8_t* raster;   /* (M, C, H, W) */
    const double* dx;        /* (M, 2) metres per pixel: [m][0] divides x, [m][1] divides y */
    int32_t M, C, H, W;
    const float* lwise;      /* (L)  */
    const float* wwise;      /* (Wc) */
    int32_t L, Wc;
    const uint32_t* raster_px4;   /* (M, H, W) copy with the 4 layers of a pixel packed into one little-endian word (byte c =
                                     layer c): one load gathers 4 layers.  Optional (NULL) for strive_map_crop_u8 and
                                     strive_coll_point, which fall back to `raster`; REQUIRED by everything that runs the fused
                                     crop -> conv1 gather (strive_map_cnn_fwd, _fwd_keep, _bwd, _bench_layer and the rollout
                                     entry points), which return an error for NULL */
} StriveMap;

/* Map CNN: 6 x [Conv2d(stride 2, pad 0) -> GroupNorm(1 group) -> ReLU] + Linear(512, 64), default
 * architecture only (kernels 7,5,5,3,3,3; channels 4->16->32->64->64->128->128; 256x256 input);
 * reference src/models/traffic_model.py:69-87, 437-440.
 * w[l]: not read by the kernels any more (all six convolutions take the fp16 fragment tables w1_frag .. w6_frag below; the
 * host side points it at w_torch[l]); kept so that the struct layout stays put;
 * fc_wt: (512, 64) transposed Linear weight. */
typedef struct StriveCNN {
    const float* w[6];
    const float* b[6];
    const float* gn_g[6];
    const float* gn_b[6];
    const float* fc_wt;
    const float* fc_b;
    const uint32_t* w1_frag;   /* layer-0 weights * wscale[0] split into two fp16 pieces (w0 = fp16(w) rounded to nearest,
                                  w1 = fp16(w - w0): w0 + w1 = w up to 2^-24 |w|) in MFMA fragment order
                                  [ky][piece][lane 0..63][8 x fp16], 8 values = window columns 2g,2g+1 x 4 layers for
                                  lane group g = lane/16, output channel = lane%16; 14336 bytes */
    const uint32_t* w2_frag;   /* layer-1 (16->32, 5x5), layer-2 (32->64, 5x5) and layer-3 (64->64, 3x3) weights, each * wscale[l] */
    const uint32_t* w3_frag;   /* and split into two fp16 pieces, in the fragment order of conv_bf6_kernel: [pass = ci/8][step s][co/32] */
    const uint32_t* w4_frag;   /* (w5_frag, w6_frag: layers 4 and 5, 64->128 and 128->128, 3x3, same format)  [piece 2][lane 64][8 x fp16]; lane half h = lane/32 holds one window tap of the step, element
                                  e = input channel 8*pass + e, output channel = 32*(co/32) + lane%32.
                                  5x5 (13 steps): tap (s/2, (s&1)+2h) for s < 10, (2(s-10)+h, 4) for s = 10, 11, (4, 4) or zero
                                  for s = 12.  3x3 (5 steps): (s, 2h) for s < 3, (h, 1) for s = 3, (2, 1) or zero for s = 4.
                                  53248 / 212992 / 163840 / 327680 / 655360 bytes */
    const uint32_t* w5_frag;
    const uint32_t* w6_frag;
    const float* w_torch[6];   /* the convolution weights in torch layout (co, ci, ky, kx): read by the training backward's
                                  data-gradient kernel only (may be NULL on the latent-optimisation path) */
    float wscale[6];           /* power of two the fp16 weight pieces of layer l were multiplied by (so that both pieces sit
                                  in fp16's normal range) */
    float xscale[6];           /* power of two the GroupNorm+ReLU input of layer l (l >= 1) is multiplied by before its fp16
                                  split; chosen from the bound |gamma| sqrt(C H W) + |beta| so that it cannot overflow */
    int32_t conv2_plain;       /* (ABI 14) conv2 normally runs as ONE persistent workgroup per CU (specialised producer / consumer
                                  waves).  A caller that runs small latency-bound kernels on a second stream under the CNN (the
                                  planner rollout behind one decoder rollout while the other rollout's CNN runs, reference
                                  src/utils/adv_gen_optim.py:133-139) passes a descriptor with conv2_plain != 0 for those calls:
                                  the ordinary conv2 kernel.  The two kernels write bit-identical activations; their GroupNorm
                                  partial sums are added in a different order (8 rows against 4 row pairs per tile), so later
                                  layers agree to fp32 rounding, not bit for bit.  A field of the caller's descriptor, not a
                                  switch inside the library: no global mutable state. */
} StriveCNN;

/* Scene structure of a batch: agents of scene b are rows ptr[b] .. ptr[b+1]-1, ego first
 * (reference src/datasets/nuscenes_dataset.py:678-702, PyG Batch.ptr).  With NS > 1 every per-agent
 * tensor has rows r = agent * NS + sample (the reference's (NA, NS, .) layout flattened). */
typedef struct StriveScenes {
    int32_t NA, NS, B;
    int32_t max_n;            /* largest scene size (host-known; sizes per-edge scratch) */
    int64_t n_edges;          /* (ABI 14) sum over scenes of n (n - 1) NS directed edge rows (host-known; sizes the training sweep's
                                 per-edge row tapes exactly instead of NA NS max_n) */
    const int32_t* ptr;       /* (B+1) */
    const int32_t* scene_of;  /* (NA)  */
} StriveScenes;

/* Everything the decoder rollout needs besides per-call tensors.
 * The width of decoder_net's last layer (gnn.mlp_out.dims[3]) selects the output model: 2 = (acceleration, yaw rate) through the
 * kinematic bicycle model (output_bicycle=True); 4 = each step's local pose (x, y, hx, hy) in the frame of the previous global
 * pose, heading normalised (output_bicycle=False, reference src/models/traffic_model.py:655-682).  With 4 outputs the bicycle
 * fields (a_mean .. max_s) are ignored and scene_par may be NULL (it is not used: direct-output rollouts run on the
 * launch-per-phase kernels). */
typedef struct StriveDecoder {
    StriveGNN gnn;
    StriveGRU gru;
    StriveCNN cnn;
    StriveMap map;
    float state_mean[6], state_std[6];   /* (x,y,hx,hy,s,hdot) normaliser, datasets/utils.py:44-113 */
    float att_mean[2], att_std[2];       /* (l,w) normaliser */
    float a_mean, a_std, ddh_mean, ddh_std, dt, max_hdot, max_s;   /* NUSC_BIKE_PARAMS, datasets/utils.py:121-127 (bicycle only) */
    /* optional (ABI 14; NULL = the scene-resident kernels are not used; laid out for a 2-output decoder only): the small parameters of decoder_net / decoder_memory in
     * one block of 6340 floats that those kernels copy to LDS -- offsets in floats (csrc/scene_rollout.h Par):
     * mlp_in  b0 0, b1 128, b2 256, ln_g0 320, ln_b0 448, ln_g1 576, ln_b1 704;
     * edge    b0 832, b1 960, b2 1088, ln_g0 1152, ln_b0 1280, ln_g1 1408, ln_b1 1536, W_rel^T (4,128) = rows 128+2NC.. of wt[0] 1664;
     * update  b0 2176, b1 2304, ln_g0 2368, ln_b0 2496;
     * mlp_out b0 2624, b1 2752, b2 2880 (2 + 2 pad), ln_g0 2884, ln_b0 3012, ln_g1 3140, ln_b1 3268, w[2] (2,128) 3396;
     * GRU     b_ih (3,192) 3652, b_hh (3,192) 4228, wih_t[0] (4,192) 4804, wih[0] (192,4) 5572. */
    const float* scene_par;
} StriveDecoder;

/* ------------------------------------------------------------------------------------------------
 * Map raster lookups
 * ---------------------------------------------------------------------------------------------- */

/* get_map_obs (reference src/datasets/nuscenes_utils.py:234-264) via NuScenesMapEnv.get_map_crop
 * (src/datasets/map_env.py:168-203).  pos (N,4) is used as pos*pos_std + pos_mean (pass 1/0 for
 * already-unnormalised frames); mapix (N) selects the map.  out: (N, C, L, Wc) uint8, bit-exact. */
int strive_map_crop_u8(const StriveMap* map, const float* pos, const float* pos_mean4_host,
                       const float* pos_std4_host, const int32_t* mapix, int32_t N, uint8_t* out,
                       strive_stream_t stream);

/* NuScenesMapEnv.__init__'s rasterisation (reference src/datasets/map_env.py:79-166): one layer of one map from polygon / line
 * geometry.  THE REFERENCE TAKES THE GEOMETRY AND ITS RASTERISER FROM THE nuscenes DEVKIT (NuScenesMap.get_map_mask ->
 * cv2.fillPoly / cv2.polylines), which is not installed here and cannot be: no fixture of its output can exist, so this entry
 * point is pinned to its own stated rule by an exact rational-arithmetic oracle (oracle/raster.py), not to the devkit.
 * Rule: pixel (r, c) = the layer's value at the world point the crop looks it up for, (c dx_x, r dx_y) (get_map_obs reads
 * raster[round(y / dx_y), round(x / dx_x)], nuscenes_utils.py:250-263): 1 inside or on the boundary of a polygon (even-odd over the
 * rings of a shape = holes) or within half_width of a polyline.  Sets bytes to 1, never clears: the caller zero-fills the layer, and
 * several jobs may target one layer (the reference collapses the road layers into channel 0, :108-113).
 * Tables (device, built by the host): shapes s = rings ring_ptr[shape_ptr[s] .. shape_ptr[s+1]]; ring r = vertices
 * verts[ring_ptr[r] .. ring_ptr[r+1]] (x, y in metres, float64; polygon rings close implicitly); shape_kind[s] 0 = polygon, 1 = line;
 * tile t = 32 x 32 pixels, row-major over ceil(H/32) x ceil(W/32): the shapes whose bounding box (grown by half_width) touches it are
 * tile_shapes[tile_ptr[t] .. tile_ptr[t+1]].  flip_rows: write row H-1-r (the reference flips the Singapore maps about the x axis,
 * :125-127).  out_layer (H, out_pitch) uint8. */
typedef struct StriveRasterJob {
    const double* verts;
    const int32_t* ring_ptr;
    const int32_t* shape_ptr;
    const uint8_t* shape_kind;
    const int32_t* tile_ptr;
    const int32_t* tile_shapes;
    int32_t H, W, out_pitch, flip_rows;
    double dx_x, dx_y, half_width;
} StriveRasterJob;

int strive_map_rasterize(const StriveRasterJob* job, uint8_t* out_layer, strive_stream_t stream);

/* get_coll_point (reference src/datasets/nuscenes_utils.py:334-390) on raster layer 0.
 * cars (N,4) unnormalised, lw (N,2); gl/gw = grid size (host computes it from the batch mean like the
 * reference, lines 351-354); lin_l (gl), lin_w (gw) = fp32 linspace(-1,1,.) tables.
 * out_pt (N,2): collision point or NaN; out_cnt (N) int32: number of non-drivable samples. */
int strive_coll_point(const StriveMap* map, const float* cars, const float* lw, const int32_t* mapix,
                      int32_t N, int32_t gl, int32_t gw, const float* lin_l, const float* lin_w,
                      float* out_pt, int32_t* out_cnt, strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Map CNN (crop fused into the first convolution)
 * ---------------------------------------------------------------------------------------------- */

size_t strive_map_cnn_workspace_bytes(int32_t N);

/* encode_map (reference src/models/traffic_model.py:416-451): feat (N,64) for N poses. */
int strive_map_cnn_fwd(const StriveMap* map, const StriveCNN* cnn, const float* pos,
                       const float* pos_mean4_host, const float* pos_std4_host, const int32_t* mapix,
                       int32_t N, float* feat, void* ws, size_t ws_bytes, strive_stream_t stream);

/* The same CNN on an explicit crop (N,4,256,256) uint8 -- for parity tests of the convolution stack. */
int strive_map_cnn_fwd_from_crop(const StriveCNN* cnn, const uint8_t* crop, int32_t N, float* feat,
                                 void* ws, size_t ws_bytes, strive_stream_t stream);

/* Measurement hook for bench.py: launch ONE kernel of the stack (layer 0 = fused crop+conv1, 1..3 = conv2..4,
 * 7 = the fused conv5 + conv6 + Linear kernel strive_map_cnn_fwd runs; 4, 5, 6 = the separate conv5 / conv6 /
 * GroupNorm+Linear kernels of the training recompute, in that order) on the activations a previous
 * strive_map_cnn_fwd over the same N poses left in `ws`, so a single kernel can be timed with events on the
 * launching stream. */
int strive_map_cnn_bench_layer(const StriveMap* map, const StriveCNN* cnn, int32_t layer, const float* pos,
                               const float* pos_mean4_host, const float* pos_std4_host, const int32_t* mapix,
                               int32_t N, float* feat, void* ws, size_t ws_bytes, strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Small operators
 * ---------------------------------------------------------------------------------------------- */

/* MLP.forward (reference src/models/common.py:41-44): y (rows, dims[nlayers]). */
int strive_mlp_fwd(const StriveMLP* mlp, const float* x, int32_t rows, float* y, strive_stream_t stream);

size_t strive_gnn_workspace_bytes(const StriveGNN* gnn, const StriveScenes* sc);

/* SceneInteractionNet.forward (reference src/models/interaction_net.py:52-77) on clique scenes.
 * x (R, mlp_in.dims[0]), pos (R,4) [NaN poses give a zero relative pose, :162], sem (NA,NC);
 * out (R, mlp_out out dim).  R = NA*NS. */
int strive_gnn_fwd(const StriveGNN* gnn, const StriveScenes* sc, const float* x, const float* pos,
                   const float* sem, float* out, void* ws, size_t ws_bytes, strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Decoder rollout (forward, and backward to the latents)
 * ---------------------------------------------------------------------------------------------- */

size_t strive_rollout_tape_bytes(const StriveDecoder* dec, const StriveScenes* sc, int32_t FT);
size_t strive_rollout_workspace_bytes(const StriveDecoder* dec, const StriveScenes* sc, int32_t FT);

/* 1 when strive_rollout_fwd / strive_rollout_bwd will run this batch on the scene-resident kernels (one workgroup per scene:
 * a decoder step is ONE launch, the reverse sweep over all FT steps is ONE launch; csrc/scene_rollout.h) -- single-sample
 * rollouts, scenes of <= 16 agents, weight packs with matrix-core fragments (StriveMLP.wf / StriveGRU.whh_f) -- else 0: the
 * launch-per-phase kernels.  Same arithmetic scheme, same tape layout; results agree to fp32 rounding.  Option
 * scene_kernels = 0 (read per call) forces 0.  2 (round 6): a single-sample batch with scenes of more than 16 agents -- the node-level
 * phases of the forward step (mlp_in .. edge partials; update MLP .. GRU .. dynamics) run on the scene kernel in 16-row tiles of
 * every scene, the edge rows and the reverse sweep on the launch-per-phase kernels (option scene_tiles = 0: all per-phase).
 * Always 0 for a direct-output decoder (4 outputs): its rollouts run on the launch-per-phase kernels at every scene size. */
int strive_rollout_scene_resident(const StriveDecoder* dec, const StriveScenes* sc);

/* TrafficModel.autoregressive_decoder (reference src/models/traffic_model.py:589-704).
 * past_last (NA,6) normalised last past state; lw (NA,2) normalised; sem (NA,NC); past_feat, map_feat
 * (NA,64); z (R,Z) (Z: the decoder pack's latent width, see STRIVE_ZDIM); mapix (NA); ext_future (B,FT,4) normalised or
 * NULL (ego rows teacher-forced, lines 667-675).  traj (R,FT,4): normalised global (x,y,hx,hy).  tape keeps what the backward needs.
 * Direct-output decoder (4 outputs): only past_last[:, :4] is read; a teacher-forced ego row's given pose also becomes its
 * previous pose of the next step (lines 679-682), and traj holds the predicted pose before that replacement. */
int strive_rollout_fwd(const StriveDecoder* dec, const StriveScenes* sc, const float* past_last,
                       const float* lw, const float* sem, const float* past_feat, const float* map_feat,
                       const float* z, const int32_t* mapix, const float* ext_future, int32_t FT,
                       float* traj, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                       strive_stream_t stream);

/* d(loss)/dz given d(loss)/d(traj): the reverse-time sweep of SURVEY.md Appendix A (no gradient flows
 * through the map crop / CNN: the reference crops at pos.detach(), traffic_model.py:694).  Both output models (StriveDecoder). */
int strive_rollout_bwd(const StriveDecoder* dec, const StriveScenes* sc, const float* lw, const float* sem,
                       const float* z, const float* ext_future, int32_t FT, const float* d_traj,
                       float* dz, const void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                       strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Collision penalties
 * ---------------------------------------------------------------------------------------------- */

/* VehCollLoss.forward (reference src/losses/adv_gen_nusc.py:464-512) restricted to in-scene pairs.
 * traj (NA,T,4) unnormalised; cent_x (NA,5) circle centres on the length axis; rad (NA).
 * Pair enumeration: for each t, for each agent i (global order), for each j in scene(i) (ascending,
 * j == i included as an always-invalid slot): index  t*P + pair_off[i] + (j - ptr[scene(i)]),
 * P = sum_b n_b^2.  pen (T,P) = 1 - dmin/(r_i+r_j+buffer); hit (T,P) uint8 = dmin <= that distance and
 * i != j; amin (T,P) uint8 = argmin over the 25 circle pairs (ci*5+cj). */
int strive_veh_coll_fwd(const StriveScenes* sc, const int32_t* pair_off, int32_t P, const float* traj,
                        int32_t T, const float* cent_x, const float* rad, float buffer, float* pen,
                        uint8_t* hit, uint8_t* amin, strive_stream_t stream);

/* d_traj (NA,T,4) += sum over pairs of d_pen * d(pen)/d(traj) (both members of each pair). */
int strive_veh_coll_bwd(const StriveScenes* sc, const int32_t* pair_off, int32_t P, const float* traj,
                        int32_t T, const float* cent_x, const float* rad, float buffer, const float* d_pen,
                        const uint8_t* amin, float* d_traj, strive_stream_t stream);

/* interp_traj (reference src/losses/adv_gen_nusc.py:625-644): linear x`scale` up-sampling in time of (x,y,hx,hy)
 * followed by heading renormalisation.  in (N,T,4) -> out (N,TO,4), TO = T*scale.  i0,i1 (TO) int32 and w0,w1 (TO) fp32
 * are the two taps of every output step as F.interpolate(mode='linear', align_corners=False) computes them. */
int strive_interp_traj_fwd(const float* in, int32_t N, int32_t T, int32_t TO, const int32_t* i0, const int32_t* i1,
                           const float* w0, const float* w1, float* out, strive_stream_t stream);
int strive_interp_traj_bwd(const float* in, const float* d_out, int32_t N, int32_t T, int32_t TO, int32_t scale,
                           const int32_t* i0, const int32_t* i1, const float* w0, const float* w1, float* d_in,
                           strive_stream_t stream);

/* AvoidCollLoss (reference src/losses/adv_gen_nusc.py:264-341) as ONE call per direction: up-sampling (:625-644), the
 * in-scene circle penalties (:405-512), the off-road collision points and their penalty (:366-403), the prior NLL
 * (:343-364), the init-z distance and the weighted masked means -- what the reference evaluates with ~60 elementwise
 * torch operators per closure.  Constants of one batch: */
typedef struct StriveAvoidColl {
    const int32_t* pair_off;     /* (NA)  first in-scene pair slot of every agent, P slots in all */
    int32_t P;
    const float* cent_x;         /* (NA,5) circle offsets along the heading */
    const float* rad;            /* (NA)   circle radii */
    float buffer;                /* veh_coll_buffer */
    const uint8_t* pair_valid;   /* (P)    1 = the slot counts (i != j, and the single-agent filter of :281-286) */
    const int32_t* i0;           /* (TO)   up-sampling taps as for strive_interp_traj_fwd */
    const int32_t* i1;
    const float* w0;
    const float* w1;
    int32_t scale;               /* TO = T * scale */
    int32_t NE;                  /* agents that take the environment term (all, or one per scene) */
    const int32_t* env_agent;    /* (NE)   their agent index */
    const int32_t* env_of_agent; /* (NA)   inverse: row e of an agent, -1 if it takes no environment term */
    const float* env_lw;         /* (NE,2) unnormalised length, width */
    const int32_t* env_mapix;    /* (NE)   */
    const float* env_pdist;      /* (NE)   sqrt(l^2/4 + w^2/4) (:373) */
    int32_t gl, gw;              /* collision-point grid (nuscenes_utils.py:351-354) */
    const float* lin_l;          /* (gl) linspace(-1,1,gl) */
    const float* lin_w;          /* (gw) */
    const float* init_z;         /* (NZ,D) */
    int32_t NZ, D;               /* latent rows (NA, or one per scene when only the first agent of a scene is optimised) */
    float prior_den, init_den;   /* denominators of the two latent means: NZ and NZ for a (NZ,D) latent; NZ and NZ*D for a
                                    (NZ,1,D) one, where the reference's sum(dim=1) runs over the singleton axis (:327-330) */
    float w_veh, w_env, w_prior, w_init;   /* loss weights; a term with weight <= 0 is skipped like the reference does */
} StriveAvoidColl;

size_t strive_avoid_coll_workspace_bytes(const StriveScenes* sc, const StriveAvoidColl* h, int32_t T);

/* traj (NA,T,4) unnormalised, z / mu / var (NZ,D).  out (8 floats): loss, mean colliding-pair penalty, mean off-road
 * penalty, mean prior NLL, mean init-z distance, #colliding valid slots, #rows with a collision point, 0.
 * `ws` keeps what the backward needs and must stay untouched until it ran. */
int strive_avoid_coll_fwd(const StriveScenes* sc, const StriveMap* map, const StriveAvoidColl* h, const float* traj,
                          int32_t T, const float* z, const float* mu, const float* var, float* out, void* ws,
                          size_t ws_bytes, strive_stream_t stream);

/* d_loss: one float ON THE DEVICE.  d_traj (NA,T,4) and d_z (NZ,D) are overwritten. */
int strive_avoid_coll_bwd(const StriveScenes* sc, const StriveAvoidColl* h, const float* traj, int32_t T, const float* z,
                          const float* mu, const float* var, const float* d_loss, void* ws, size_t ws_bytes,
                          float* d_traj, float* d_z, strive_stream_t stream);

/* AdvGenLoss (reference src/losses/adv_gen_nusc.py:53-262) as one call per direction.  `base` carries what it shares with
 * AvoidCollLoss: the pair penalties (pair_valid = i != j), the up-sampling taps, the environment term over the NON-EGO agents
 * (env_agent = their agent indices, NE = NA - B; the latent tensors z / mu / var / init_z have one row per non-ego agent in
 * the same order, so base.NZ = NE) and the latent size.  base.w_veh / w_env / w_prior / w_init are the weights 'coll_veh',
 * 'coll_env', 'motion_prior', 'init_z'; base.prior_den = NE, base.init_den is unused (the init term is a plain sum, :216-223). */
typedef struct StriveAdvGen {
    StriveAvoidColl base;
    const int32_t* ne_ptr;       /* (B+1)  offsets of every scene's non-ego agents in the non-ego order */
    const int32_t* slot_ne;      /* (P)    non-ego row of the non-ego member of a pair slot that involves the scene's ego, else -1 */
    const uint8_t* atk_mask;     /* (NE)   1 = may be the attacker (attack_agt_idx, :126-130), or NULL = everybody */
    const uint8_t* scene_alive;  /* (B) or NULL.  0 = the scene has left the batch (closed loop: its planner rollout failed,
                                    strive_planner_rollout's `alive`): it contributes to no sum and no count -- colliding pairs,
                                    off-road rows, prior / init rows, crash term, the 1/NE and 1/B of the two means -- and receives
                                    zero gradients; the other scenes get exactly the values of the batch rebuilt without it
                                    (the reference's remedy for scenes it gives up, adv_scenario_gen.py:323-356) */
    int32_t t0;                  /* crash_loss_min_time */
    int32_t use_infront;         /* crash_loss_min_infront given? */
    float infront;
    float w_crash, w_plan, w_prior_atk, w_init_atk;   /* 'adv_crash', 'coll_veh_plan', 'motion_prior_atk', 'init_z_atk' */
} StriveAdvGen;

size_t strive_adv_gen_workspace_bytes(const StriveScenes* sc, const StriveAdvGen* h, int32_t T);

/* traj (NA,T,4) and tgt (B,T,4) unnormalised; z / mu / var (NE,D).  out (16 floats): loss, mean colliding non-ego pair
 * penalty, mean weighted planner-pair penalty, mean off-road penalty, mean weighted prior NLL, weighted init-z sum, mean crash
 * term, the four counts (pairs, planner pairs, off-road rows, 1 if every attacker was always behind its target), 0...
 * soft (NE, T - t0): the per-scene soft-min weights (:133-135), rew (NE): 1 - their sum per agent. */
int strive_adv_gen_fwd(const StriveScenes* sc, const StriveMap* map, const StriveAdvGen* h, const float* traj, const float* tgt,
                       int32_t T, const float* z, const float* mu, const float* var, float* out, float* soft, float* rew,
                       void* ws, size_t ws_bytes, strive_stream_t stream);

/* d_loss: one float on the device.  d_traj (NA,T,4), d_tgt (B,T,4) and d_z (NE,D) are overwritten. */
int strive_adv_gen_bwd(const StriveScenes* sc, const StriveAdvGen* h, const float* traj, const float* tgt, int32_t T,
                       const float* z, const float* mu, const float* var, const float* d_loss, void* ws, size_t ws_bytes,
                       float* d_traj, float* d_tgt, float* d_z, strive_stream_t stream);

/* strive_coll_point over the rows (e, t) of an up-sampled trajectory tensor without expanding the per-agent attributes:
 * car = fine[agent_of[e]*TO + t], size lw[e], map mapix[e]; out_pt (NE*TO,2), out_cnt (NE*TO). */
int strive_coll_point_rows(const StriveMap* map, const float* fine, int32_t TO, const int32_t* agent_of, const float* lw,
                           const int32_t* mapix, int32_t NE, int32_t gl, int32_t gw, const float* lin_l,
                           const float* lin_w, float* out_pt, int32_t* out_cnt, strive_stream_t stream);

/* Rotated-rectangle IoU of P box pairs (x, y, hx, hy) + (l, w), float64 out; NaN where a pose contains NaN.
 * Replaces the shapely polygon loop of check_single_veh_coll / check_pairwise_veh_coll
 * (reference src/losses/adv_gen_nusc.py:517-623; corners as src/datasets/nuscenes_utils.py:416-428). */
int strive_rect_iou(const float* box_a, const float* lw_a, const float* box_b, const float* lw_b, int32_t P, double* iou,
                    strive_stream_t stream);

/* Planner evaluation metrics (reference src/eval_planner.py:114-218, compute_metrics) of B scenes in ONE launch, float64:
 * x`scale` up-sampling of the plan (float64) and of the other agents (fp32; NaN = unobserved) as interp_traj
 * (reference src/losses/adv_gen_nusc.py:625-644, taps restated in the kernel), the IoU of the ego box against every other
 * agent at every fine step (hit: IoU > 0.02, NaN frames skipped, :517-565), the earliest hit and the lowest agent index
 * attaining it (np.amin / np.argmin), coll_idx = int((coll_time * (dt / scale)) / dt) or T-1, the relative speed at impact
 * and the acceleration series of the pre-crash frames.  The ego is NOT among ``others``.
 *   plan (B,T,4) float64, others (NR,T,4), ptr (B+1) offsets into others, lw_ego (B,2), lw_others (NR,2)
 *   out_i (B,5) int32 : did_collide, coll_time (T*scale without a hit), coll_agt, coll_idx, number of acceleration frames
 *   out_d (B,7) double: coll_vel (NaN without a hit), then (sum, max) of |accel|, forward accel, lateral accel
 *   status (B) int32  : 0 = written; 1 = the scene has no other agent, 2 = its offsets leave ``others`` (outputs untouched)
 * A scene's outputs are bit-identical whatever else is in the batch.  T >= 2, scale >= 1. */
int strive_planner_eval_metrics(const double* plan, const float* others, const int32_t* ptr, const float* lw_ego,
                                const float* lw_others, int32_t B, int32_t NR, int32_t T, int32_t scale, double dt,
                                int32_t* out_i, double* out_d, int32_t* status, strive_stream_t stream);

/* Adversarial-scenario evaluation (reference src/eval_adv_gen.py:339-513 compute_metrics and :116-168 compute_coll_feat) of
 * B scenes in ONE launch, float64 on the fp32 inputs, one workgroup per scene.
 *   fut (NA,T,4) every scene's fut_adv, the ego first; ptr (B+1) offsets into fut / lw / z; lw (NA,2); atk_agt (B) the JSON's
 *   attack_agt; dt (B); z, mu, var (NA,D), D = 1..64, or all three NULL (no log-likelihood); plan_fit (B,T,4) the
 *   fut_internal_ego rows read where has_fit (B) is set; map + mapix (B) + lin_tab, or a NULL map (no environment terms);
 *   lin_tab holds the fp32 linspace(-1, 1, k) tables for k = 1..lin_max one after the other (table k starts at k(k-1)/2);
 *   want_feat (B) asks for the collision features.
 * Per scene: the ego against every other agent at the coarse steps (check_single_veh_coll, reference
 * src/losses/adv_gen_nusc.py:517-565; hit = IoU > 0.02, NaN frames skipped) -> adv_collide, coll_t = amin of the first-hit
 * times (T without a hit), coll_agt = argmin + 1; the effective attacker is coll_agt after a hit, else atk_agt, the "others"
 * every agent but the ego and that attacker.  With coll_t > 0: check_pairwise_veh_coll (:567-623) on the non-ego agents over
 * [0, coll_t) -- the reference's early breaks make its coll_count the number of agents i overlapping some j > i at some
 * step -- and, with a map, compute_coll_rate_env_from_traj (src/losses/traffic_model.py:421-463) / check_on_layer
 * (src/datasets/nuscenes_utils.py:266-298) with the grid L = round(mean_l / mean(dx)) from the scene's valid rows.  Then
 * compute_accels (:323-337) over [0, coll_t) for the attacker (coll_t > 2) and the others, log_normal
 * (src/losses/common.py:26-42) of the attacker's and the others' latents, the planner fit over [0, coll_t), and the
 * collision features at the first x5 up-sampled contact (transform2frame, src/utils/transforms.py:78-139).
 *   out_i (B,20) int32 : adv_collide, coll_t, coll_agt, atk_agt, num_coll_veh, num_traj_veh, env_coll_atk, env_coll_others,
 *                        n_others, env_L, env_W, atk_accel_cnt, other_accel_cnt, ll_other_cnt, fit_cnt, feat_status (-1 not
 *                        asked, 0 found, 1 no fine-step contact), fine_t, fine_agt, lr_coll_t, env_frames; -1 = absent
 *   out_d (B,26) double: (sum, max) of |accel|, forward, lateral for the attacker, the same six for the others, ll_atk,
 *                        ll_other_sum, fit_pos_sum, fit_ang_rad_sum, fit_ang_deg_sum, hvec (2), angvec (2), h, ang, rel_s,
 *                        env_mean_l, env_mean_w; NaN = absent
 *   status (B) int32   : 0 = written; 1 = ego only; 2 = offsets, attack_agt or map index out of range; 3 = more than 63
 *                        others; 4 = the sampling grid exceeds lin_max (outputs untouched for every non-zero status)
 * A scene's outputs are bit-identical whatever else is in the batch.  T >= 2. */
int strive_scenario_eval_metrics(const float* fut, const int32_t* ptr, const float* lw, const int32_t* atk_agt, const double* dt,
                                 const float* z, const float* mu, const float* var, int32_t D, const float* plan_fit,
                                 const int32_t* has_fit, const StriveMap* map, const int32_t* mapix, const float* lin_tab,
                                 int32_t lin_max, const int32_t* want_feat, int32_t B, int32_t NA, int32_t T, int32_t* out_i,
                                 double* out_d, int32_t* status, strive_stream_t stream);

/* Traffic-model evaluation metrics (reference src/test_traffic.py:84-277 with compute_err, compute_disp_err,
 * compute_coll_rate_env and compute_coll_rate_veh of reference src/losses/traffic_model.py:120-164, :297-364, :366-419,
 * :465-545) for ONE prediction set of B scenes in one host call without a host synchronisation; float64 on the fp32 inputs,
 * one workgroup per scene (up to 8 with many samples: a scene's (agent, sample) flags are dealt out, each has one owner),
 * preceded by a one-workgroup launch that forms the batch-wide sampling grid when env is asked for.
 *   pred (NA,NS,T,4), gt (NA,Tg,6) and lw (NA,2) NORMALISED, unnormalised in fp32 as v * std + mean (MeanStdNormalizer,
 *   reference src/datasets/utils.py:75-90) with the four host arrays; vis (NA,Tg) fp32; ptr (B+1) agent offsets, the ego first;
 *   map + mapix (B) + lin_tab / lin_max as for strive_scenario_eval_metrics (env only); groups = 1 err | 2 disp | 4 veh |
 *   8 env | 16 use the caller's grid_i instead of forming it; env_ego_only as the reference's ego_only.
 *   err : pos_err, ang_err (NA,Tg) of sample 0, NaN where vis != 1, degrees (needs T == Tg)
 *   disp: (B,5) pos_minADE, pos_minFDE, ang_minADE, ang_minFDE, APD of the scene's ego over min(T, Tg) steps (APD NaN for NS 1)
 *   veh : did_veh (NA,NS) int32, agent i overlaps (IoU > 0.02) an agent j > i of its scene at some step; NaN frames never hit
 *   env : did_map (B,NS) with env_ego_only else (NA,NS) int32, some valid frame has fp32(count) / fp32(L W) < fp32(0.95) on
 *         raster layer 0 (check_on_layer, reference src/datasets/nuscenes_utils.py:266-298); L = round(mean_l / mean(dx)), W
 *         likewise over the valid (agent, sample, step) rows of the whole call (ego rows only with env_ego_only);
 *         grid_i (3) = L, W, valid rows (clamped); grid_d (2) = the two ratios before rounding (NaN without a valid row)
 *   status (B) int32: 0 = written; 2 = offsets leave the arrays; 3 = map index out of range; 4 = the grid is outside
 *         1..lin_max (outputs untouched for every non-zero status).  A group that is not asked for leaves its outputs
 *         untouched and may pass NULL for them.
 * Given the grid, a scene's outputs are bit-identical whatever else is in the batch. */
int strive_traffic_eval_metrics(const float* pred, const float* gt, const float* vis, const int32_t* ptr, const float* lw,
                                const float* state_mean4_host, const float* state_std4_host, const float* att_mean2_host,
                                const float* att_std2_host, const StriveMap* map, const int32_t* mapix, const float* lin_tab,
                                int32_t lin_max, int32_t groups, int32_t env_ego_only, int32_t B, int32_t NA, int32_t NS,
                                int32_t T, int32_t Tg, double* pos_err, double* ang_err, double* disp, int32_t* did_veh,
                                int32_t* did_map, int32_t* grid_i, double* grid_d, int32_t* status, strive_stream_t stream);

/* Collision verdicts of the refine driver (compute_metrics, reference src/refine_traffic_optim.py:84-121, with
 * check_pairwise_veh_coll of reference src/losses/adv_gen_nusc.py:567-623 and compute_coll_rate_env of reference
 * src/losses/traffic_model.py:366-419 -> check_on_layer, reference src/datasets/nuscenes_utils.py:266-298) for B scenes in one
 * host call without a host synchronisation, each scene as if compute_metrics had been called on that scene alone: two
 * launches, float64 on the fp32 inputs, any scene size.
 *   traj (NA,T,4) and lw (NA,2) NORMALISED, unnormalised in fp32 as for strive_traffic_eval_metrics with the four host arrays;
 *   ptr (B+1) agent offsets; map + mapix (B) + lin_tab / lin_max as for strive_scenario_eval_metrics.
 *   did_veh (NA) int32: agent i overlaps (IoU > 0.02) an agent j > i of its scene at some step; NaN frames never hit
 *   did_env (NA) int32: some valid frame has fp32(count) / fp32(L W) < fp32(0.95) on raster layer 0, the grid L = round(mean_l /
 *         mean(dx)), W likewise, formed from the valid (agent, step) rows of THAT SCENE (mean(dx) over all entries of the
 *         map's dx); a scene without a valid row has L = W = 0, NaN ratios and no environment collision
 *   out_i (B,8) int32 : num_coll_veh, num_traj_veh (= n), env_coll, env_total (= n), success (both counts 0), L, W, valid rows
 *   grid_d (B,2)      : the two ratios before rounding
 *   status (B) int32  : 0 = written; 2 = offsets leave the arrays or n < 1; 3 = map index out of range; 4 = this scene's grid
 *         is outside 1..lin_max (other scenes are unaffected).  Every output of a scene with a non-zero status is untouched.
 * No floating-point atomics and every sum in a fixed order: a scene's outputs are bit-identical whatever else is in the batch
 * and however many workgroups serve the scene. */
int strive_refine_verdicts(const float* traj, const int32_t* ptr, const float* lw, const float* state_mean4_host,
                           const float* state_std4_host, const float* att_mean2_host, const float* att_std2_host,
                           const StriveMap* map, const int32_t* mapix, const float* lin_tab, int32_t lin_max, int32_t B,
                           int32_t NA, int32_t T, int32_t* did_veh, int32_t* did_env, int32_t* out_i, double* grid_d,
                           int32_t* status, strive_stream_t stream);

/* Ego-against-others verdicts of the scenario generator (check_single_veh_coll, reference src/losses/adv_gen_nusc.py:517-565, with
 * what compute_adv_gen_success, reference src/utils/adv_gen_optim.py:214-235, and compute_sol_success, reference
 * src/utils/sol_optim.py:126-165, read from it) for B scenes in one launch without a host synchronisation, each scene as if judged
 * alone: float64 on the fp32 inputs, any scene size, no atomics.
 *   traj (NA,T,4) and lw (NA,2) NORMALISED, unnormalised in fp32 with the four host arrays; ptr (B+1) agent offsets, agent 0 of a
 *   scene is its ego; atk (B) the local attacker index 1..n-1 or -1, NULL = no attacker anywhere; want_env != 0 asks for the ego's
 *   drivable test and needs map + mapix (B) + lin_tab / lin_max as for strive_refine_verdicts (otherwise they may be NULL).
 *   hit (NA) int32    : the other agent overlaps the ego (IoU > 0.02) at some step; NaN frames never hit
 *   coll_t (NA) int32 : the first such step, T if none.  The ego's own row of hit / coll_t holds the scene's n_hit > 0 / first_t.
 *   out_i (B,8) int32 : n_others, n_hit, atk_hit (-1 without an attacker), first_t, ego_env (the ego's did_collide of
 *         compute_coll_rate_env(ego_only=True) on that scene alone: the grid L = round(l / mean(dx)), W likewise, from the ego's
 *         valid frames; -1 if not asked), L, W, valid ego rows
 *   grid_d (B,2)      : the two ratios before rounding (NaN if not asked or no valid ego row)
 *   status (B) int32  : 0 = written; 2 = offsets leave the arrays, n < 1, or an attacker index other than -1 outside 1..n-1;
 *         3 = map index out of range; 4 = the grid is outside 1..lin_max.  Every output of a scene with a non-zero status is untouched.
 * A scene's outputs are bit-identical whatever else is in the batch. */
int strive_ego_verdicts(const float* traj, const int32_t* ptr, const float* lw, const int32_t* atk,
                        const float* state_mean4_host, const float* state_std4_host, const float* att_mean2_host,
                        const float* att_std2_host, int32_t want_env, const StriveMap* map, const int32_t* mapix,
                        const float* lin_tab, int32_t lin_max, int32_t B, int32_t NA, int32_t T, int32_t* hit, int32_t* coll_t,
                        int32_t* out_i, double* grid_d, int32_t* status, strive_stream_t stream);

/* Feasibility screening of the scenario generator (determine_feasibility_nusc, reference src/utils/scenario_gen.py:30-107, with
 * check_line_layer, reference src/datasets/nuscenes_utils.py:300-332, and the two ego-speed rules of reference
 * src/adv_scenario_gen.py:176-195) for B scenes in one launch without a host synchronisation, each scene as if screened alone.
 *   samples (NA,NS,FT,4) NORMALISED (FT >= 2), agent 0 of a scene is its ego; gt (NA,Tg,4) NORMALISED or NULL, only each scene's ego
 *   row is read; both are unnormalised in fp32 with the two host arrays.  allowed (NA) int32 or NULL: the adv_attack_with mask.
 *   thresh (m), t0 (the first step that counts), agent_vel / ego_vel (m per step: an agent is feasible only if its largest step
 *   displacement is > agent_vel, the ego is too slow if its largest is < ego_vel), use_infront + infront_min in [-1,1] (a step
 *   counts only if cos(ego heading, ego -> agent) >= infront_min; coincident positions do not count), check_sep, planner_rule (which
 *   ego speed decides verdict 1: 0 none, 1 gt, 2 the samples).
 * Distances, cosines, speeds and line lengths are float64 on the fp32 values.  The closest approach takes the minimum over the
 * samples first (the first sample on a tie), then over the steps (the first step on a tie); an agent with every step masked has
 * dist = inf, step = t0, best_samp = 0.  With check_sep the line from the agent to the ego at (best_samp, step) is sampled at
 * sep_n points start (1 - w) + end w, w = linspace(0,1,sep_n), in fp32, divided by the map's dx in float64 and rounded half to even;
 * sep_n = max over THAT SCENE's non-ego agents of round(|agent - ego| / mean(dx)) (mean over all entries of the map pack's dx).
 *   per non-ego agent (the ego's rows are untouched): feasible (within, no line sample on a 0 pixel, fast enough, allowed), within,
 *         step, best_samp, sep_zero (line samples on a 0 pixel) int32; dist, max_vel double
 *   out_i (B,8) int32 : n_others, n_within, n_feasible_any_category, n_feasible, heur_agt (local index of the feasible agent with the
 *         smallest dist, the lowest index on a tie, -1 if none), heur_t (its step, -1), sep_n, verdict: 1 = ego too slow, 2 = ego
 *         only, 3 = no vehicle near, 4 = no feasible attacker of the requested category, 0 = feasible (the reference's order)
 *   out_d (B,3)       : the ego's largest step displacement over the samples, over gt (NaN without gt or Tg < 2), heur_dist (inf if none)
 *   status (B) int32  : 0 = written; 2 = offsets leave the arrays or n < 1; 3 = map index out of range; 5 = a sample is not finite;
 *         6 = a line sample lies outside the raster (torch would raise or wrap) or sep_n > 65536.  Every output of a scene with a
 *         non-zero status is untouched.
 * No atomics; a scene's outputs are bit-identical whatever else is in the batch. */
int strive_feasibility_screen(const float* samples, const int32_t* ptr, const int32_t* mapix, const int32_t* allowed, const float* gt,
                              const float* state_mean4_host, const float* state_std4_host, const StriveMap* map, double thresh,
                              int32_t t0, double agent_vel, double ego_vel, int32_t use_infront, double infront_min,
                              int32_t check_sep, int32_t planner_rule, int32_t B, int32_t NA, int32_t NS, int32_t FT, int32_t Tg,
                              int32_t* feasible, int32_t* within, int32_t* step, int32_t* best_samp, double* dist, int32_t* sep_zero,
                              double* max_vel, int32_t* out_i, double* out_d, int32_t* status, strive_stream_t stream);

/* One Lloyd step of k-means on x (N,F) float64 with centers (k,F), F = 1..8, k = 1..64 (the clustering of reference
 * src/cluster_scenarios.py, which calls scikit-learn's KMeans on the host): labels (N) = nearest centre, the lowest index on
 * equal squared distance; mind (N) that distance; sums (k,F) and counts (k) per cluster; inertia (1) = sum of mind.  Two
 * launches; the sums are reduced in a fixed order without atomics on doubles, so two runs give the same bytes. */
int strive_kmeans_step(const double* x, const double* centers, int32_t N, int32_t F, int32_t k, int32_t* labels, double* mind,
                       double* sums, int32_t* counts, double* inertia, strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training backward (weight gradients) -- reference src/train_traffic.py:103-131 calls loss.backward() through
 * TrafficModel.forward (src/models/traffic_model.py:178-225).
 *
 * Gradient buffers are flat fp32 arrays in the parameter order of the reference module (torch named_parameters()),
 * ACCUMULATED into (the caller zeroes them):
 *   MLP  (models/common.py:8-44):      per layer l:  W_l (dims[l+1], dims[l]) | b_l | and for hidden layers LN gamma_l | beta_l
 *   GNN  (models/interaction_net.py):  mlp_in | msg.0.edge_mlp | msg.0.update_mlp | mlp_out
 *   GRU  (nn.GRU(4, 64, 3)):           per layer: weight_ih (192, in_l) | weight_hh (192, 64) | bias_ih | bias_hh
 *   CNN  (traffic_model.py:69-87):     per layer: conv W (co, ci, k, k) | conv b | GroupNorm gamma | beta;  then Linear W (64, 512) | b
 * Weight gradients are summed with fp32 atomics (their summation order is not fixed run to run); input gradients are
 * deterministic.
 * ---------------------------------------------------------------------------------------------- */
size_t strive_mlp_param_count(const StriveMLP* mlp);
size_t strive_gnn_param_count(const StriveGNN* gnn);
size_t strive_gru_param_count(void);
size_t strive_map_cnn_param_count(void);

/* MLP.forward under autograd (reference src/models/common.py:41-44): dy (rows, out) -> d_params (+=) and, if dx != NULL,
 * dx (rows, in).  The forward is recomputed from x. */
int strive_mlp_bwd(const StriveMLP* mlp, const float* x, const float* dy, int32_t rows, float* dx, float* d_params,
                   strive_stream_t stream);

/* Weight pack of one Linear layer (reference src/models/common.py:26-39 stores W (out, in)): w (M, K) fp32 on the device ->
 * wt (K, M) fp32, wf / wbf = the two-piece fp16 fragments of w * scale / w^T * scale (StriveMLP.wf / .wbf layout;
 * (M+15)/16 * (K+31)/32 * 2 KiB and (K+15)/16 * (M+31)/32 * 2 KiB).  Any output may be NULL.  One launch: the training step
 * re-packs every layer after each optimiser step. */
int strive_pack_dense(const float* w, int32_t M, int32_t K, float scale, float* wt, void* wf, void* wbf, strive_stream_t stream);

/* Any two-piece fp16 fragment table of a weight tensor in one launch: out[i] (n_out x fp16) = piece idx[i] / n_w of the split of
 * w[idx[i] % n_w] * scale, or 0 where idx[i] == 2 n_w.  The index table IS the operand layout (the convolution layouts of
 * StriveCNN.w1_frag .. w6_frag); the training step re-packs the six convolutions after each optimiser step. */
int strive_pack_split_gather(const float* w, int32_t n_w, const int32_t* idx, int32_t n_out, float scale, void* out,
                             strive_stream_t stream);

size_t strive_gnn_bwd_workspace_bytes(const StriveGNN* gnn, const StriveScenes* sc);

/* SceneInteractionNet.forward under autograd (reference src/models/interaction_net.py:52-77): d_out (R, out) ->
 * dx (R, mlp_in.dims[0]) and d_params (+=).  pos carries no gradient here (the encoders are called at data poses). */
int strive_gnn_bwd(const StriveGNN* gnn, const StriveScenes* sc, const float* x, const float* pos, const float* sem,
                   const float* d_out, float* dx, float* d_params, void* ws, size_t ws_bytes, strive_stream_t stream);

size_t strive_map_cnn_bwd_workspace_bytes(int32_t N);

/* encode_map under autograd (reference src/models/traffic_model.py:416-451; the crop is data): d_feat (N,64) at the N
 * poses `pos` -> d_params (+=).  The forward is recomputed in chunks inside. */
int strive_map_cnn_bwd(const StriveMap* map, const StriveCNN* cnn, const float* pos, const float* pos_mean4_host,
                       const float* pos_std4_host, const int32_t* mapix, int32_t N, const float* d_feat, float* d_params,
                       void* ws, size_t ws_bytes, strive_stream_t stream);

/* Measurement hook for bench.py's training line (the counterpart of strive_map_cnn_bench_layer): launch ONE kernel of the CNN
 * backward -- the data gradient of conv layer `layer` (1..5: d conv2 .. d conv6 input) -- on the buffers a previous
 * strive_map_cnn_bwd over the same N (<= 256, one backward chunk) samples left in `ws`, so it can be timed with events on the
 * launching stream.  It overwrites the gradient buffer of layer - 1 in `ws` (scratch of the finished call). */
int strive_map_cnn_bwd_bench_dgrad(int32_t layer, int32_t N, void* ws, size_t ws_bytes, strive_stream_t stream);

/* Kept activations (round 5): the training forward may keep the raw outputs of the six convolutions and their GroupNorm partial sums
 * of every crop it encodes (1.76 MB per crop) so that the backward does not run the layers again -- the reference's autograd keeps
 * ALL activations of map_conv (src/models/traffic_model.py:69-87 under loss.backward()); only the crop is gathered again.  strive_map_cnn_fwd_keep = strive_map_cnn_fwd that also writes rows [kept_offset, kept_offset + N) of a kept buffer
 * sized for kept_total crops (strive_map_cnn_keep_bytes(kept_total)); strive_map_cnn_bwd_kept = strive_map_cnn_bwd over the N =
 * kept_total crops of such a buffer, in the buffer's row order. */
size_t strive_map_cnn_keep_bytes(int32_t N);
int strive_map_cnn_fwd_keep(const StriveMap* map, const StriveCNN* cnn, const float* pos, const float* pos_mean4_host,
                            const float* pos_std4_host, const int32_t* mapix, int32_t N, float* feat, void* ws, size_t ws_bytes,
                            void* kept, size_t kept_bytes, int32_t kept_total, int32_t kept_offset, strive_stream_t stream);
int strive_map_cnn_bwd_kept(const StriveMap* map, const StriveCNN* cnn, const float* pos, const float* pos_mean4_host,
                            const float* pos_std4_host, const int32_t* mapix, int32_t N, const float* d_feat, float* d_params,
                            const void* kept, size_t kept_bytes, void* ws, size_t ws_bytes, strive_stream_t stream);

/* ... over rows [kept_offset, kept_offset + N) of a kept buffer sized for kept_total crops; pos / mapix / d_feat point at the first
 * of these rows (strive_rollout_bwd_train_kept hands the crops of a few steps at a time to a side stream while its sweep continues). */
int strive_map_cnn_bwd_kept_range(const StriveMap* map, const StriveCNN* cnn, const float* pos, const float* pos_mean4_host,
                                  const float* pos_std4_host, const int32_t* mapix, int32_t N, const float* d_feat, float* d_params,
                                  const void* kept, size_t kept_bytes, int32_t kept_total, int32_t kept_offset, void* ws,
                                  size_t ws_bytes, strive_stream_t stream);

size_t strive_rollout_train_workspace_bytes(const StriveDecoder* dec, const StriveScenes* sc, int32_t FT);

/* strive_rollout_fwd keeping the map CNN's activations of its FT - 1 re-encoded steps in `kept` (strive_rollout_keep_bytes), and
 * strive_rollout_bwd_train reading them instead of recomputing (same results; the tape and `kept` belong to one forward call). */
size_t strive_rollout_keep_bytes(const StriveDecoder* dec, const StriveScenes* sc, int32_t FT);
int strive_rollout_fwd_keep(const StriveDecoder* dec, const StriveScenes* sc, const float* past_last, const float* lw,
                            const float* sem, const float* past_feat, const float* map_feat, const float* z, const int32_t* mapix,
                            const float* ext_future, int32_t FT, float* traj, void* tape, size_t tape_bytes, void* ws,
                            size_t ws_bytes, void* kept, size_t kept_bytes, strive_stream_t stream);
int strive_rollout_bwd_train_kept(const StriveDecoder* dec, const StriveScenes* sc, const float* lw, const float* sem,
                                  const float* z, const float* ext_future, const int32_t* mapix, int32_t FT, const float* d_traj,
                                  float* dz, float* d_past_feat, float* d_map_feat, float* d_gnn, float* d_gru, float* d_cnn,
                                  const void* tape, size_t tape_bytes, const void* kept, size_t kept_bytes, void* ws,
                                  size_t ws_bytes, strive_stream_t stream);

/* autoregressive_decoder under autograd with parameter gradients (reference src/models/traffic_model.py:589-704 as used
 * by forward(), :178-225): like strive_rollout_bwd, plus d_past_feat, d_map_feat (NA,64) -- the adjoints of the encoder
 * outputs the rollout starts from -- and the gradients of decoder_net (d_gnn), decoder_memory (d_gru) and of the map CNN
 * (d_cnn: every step t >= 1 re-encodes the map at the detached pose, :694-695), all (+=).  NS must be 1.  Both output models
 * (StriveDecoder): d_gnn's last mlp_out layer is (2,128) + 2 or (4,128) + 4. */
int strive_rollout_bwd_train(const StriveDecoder* dec, const StriveScenes* sc, const float* lw, const float* sem,
                             const float* z, const float* ext_future, const int32_t* mapix, int32_t FT, const float* d_traj,
                             float* dz, float* d_past_feat, float* d_map_feat, float* d_gnn, float* d_gru, float* d_cnn,
                             const void* tape, size_t tape_bytes, void* ws, size_t ws_bytes, strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GRU trajectory encoders (traj_encoder='gru'; reference src/models/traffic_model.py:93-119, 453-523): past / future encoder =
 * nn.GRU(in, 128, num_layers=4, batch_first=True) over the T frames of every agent, zero initial state, gate order r, z, n
 * (n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h' = (1 - z) n + z h), then nn.Linear(128, 64) on the top layer's last state.
 * ---------------------------------------------------------------------------------------------- */
#define STRIVE_TGRU_LAYERS 4
#define STRIVE_TGRU_HID 128
#define STRIVE_TGRU_MAX_IN 32

/* wih[l] (384, in_l) with in_0 = in_size, in_l = 128 otherwise, whh[l] (384, 128): torch layouts; bih[l], bhh[l] (384).
 * Matrix-core operands (all required; StriveMLP.wf layout, two fp16 pieces): wih_f[l] / whh_f[l] = fragments of wih[l] * ih_sc[l] /
 * whh[l] * hh_sc[l] (rows = the 384 gate outputs); wih_bf[l][q] / whh_bf[l][q] = fragments of the TRANSPOSE of gate block q
 * (rows 128 q .. 128 q + 127 of the matrix, q = r, z, n) times the same scale: rows = the layer's inputs, k = the 128 outputs of the
 * gate -- the input-gradient products of the backward, one per gate.  wih_bf[0] is not read (no gradient reaches the sequence).
 * out_w (64, 128), out_b (64): the Linear; out_wf / out_wbf its fragments and those of its transpose, times out_sc.
 * Scales are powers of two. */
typedef struct StriveTrajGRU {
    int32_t in_size;          /* NC + 9, at most STRIVE_TGRU_MAX_IN */
    int32_t reserved;
    const float* wih[STRIVE_TGRU_LAYERS];
    const float* whh[STRIVE_TGRU_LAYERS];
    const float* bih[STRIVE_TGRU_LAYERS];
    const float* bhh[STRIVE_TGRU_LAYERS];
    const void* wih_f[STRIVE_TGRU_LAYERS];
    const void* whh_f[STRIVE_TGRU_LAYERS];
    const void* wih_bf[STRIVE_TGRU_LAYERS][3];
    const void* whh_bf[STRIVE_TGRU_LAYERS][3];
    float ih_sc[STRIVE_TGRU_LAYERS];
    float hh_sc[STRIVE_TGRU_LAYERS];
    const float* out_w;
    const float* out_b;
    const void* out_wf;
    const void* out_wbf;
    float out_sc;
} StriveTrajGRU;

/* encode_past / encode_future with traj_encoder='gru' (reference src/models/traffic_model.py:477-486, 513-523) on the assembled
 * sequence x (NA, T, in_size): feat (NA, 64).  ONE launch runs all T steps and all 4 layers; T is a run-time argument.
 * T < 1 and in_size > STRIVE_TGRU_MAX_IN are refused. */
int strive_traj_gru_fwd(const StriveTrajGRU* gru, const float* x, int32_t NA, int32_t T, float* feat, strive_stream_t stream);

/* Training: strive_traj_gru_fwd_keep = strive_traj_gru_fwd (same bytes in feat) that also writes what the backward needs into
 * `kept` (strive_traj_gru_keep_bytes: the input rows, every layer-step's gates r, z, n, W_hn h + b_hn and new state, and the
 * backward's own scratch, so `kept` is read AND written by strive_traj_gru_bwd).  strive_traj_gru_bwd: d_feat (NA, 64) ->
 * d_params (+=), strive_traj_gru_param_count floats in the order of the reference modules' named_parameters(): per layer
 * weight_ih | weight_hh | bias_ih | bias_hh, then the Linear's weight | bias.  The weight gradients are deferred products over
 * the rows of all steps (WJobTable), not per-step atomics.  No gradient with respect to x: the reference's graph ends at the
 * data (src/models/traffic_model.py:465-478). */
size_t strive_traj_gru_param_count(const StriveTrajGRU* gru);
size_t strive_traj_gru_keep_bytes(const StriveTrajGRU* gru, int32_t NA, int32_t T);
int strive_traj_gru_fwd_keep(const StriveTrajGRU* gru, const float* x, int32_t NA, int32_t T, float* feat, void* kept,
                             size_t kept_bytes, strive_stream_t stream);
int strive_traj_gru_bwd(const StriveTrajGRU* gru, int32_t NA, int32_t T, void* kept, size_t kept_bytes, const float* d_feat,
                        float* d_params, strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Rule-based lane-following planner (reference src/planners/hardcode_goalcond_nusc.py), the planner that
 * adv_gen_rule_based.cfg attacks in closed loop: src/utils/adv_gen_optim.py:133-139 calls
 * HardcodeNuscPlanner.rollout once per optimisation iteration.  All arithmetic is float64 like the reference's numpy.
 * ---------------------------------------------------------------------------------------------- */
#define STRIVE_PLANNER_MAXMAPS 4
#define STRIVE_PLANNER_NSTATUS 8

/* Connections of one lane-graph node in list order (out_edges / in_edges of the reference's lane-graph dict,
 * src/datasets/nuscenes_utils.py:50-123), the first four inline; len = |xy[node] - xy[this]|. */
typedef struct StriveLaneNode {
    int32_t n;
    int32_t node[4];
    int32_t pad[3];
    double len[4];
} StriveLaneNode;

/* One map's lane graph + a uniform grid over its directed edges (each edge is listed, in ascending order, in every cell
 * its bounding box grown by `xydistmax` touches, so that get_lane_matches (:298-322) reads one cell instead of all edges). */
typedef struct StrivePlannerMap {
    const double* xy;                 /* (N,2) node positions */
    const StriveLaneNode* succ;       /* (N) */
    const StriveLaneNode* pred;       /* (N) */
    const int32_t* succ_ptr;          /* (N+1)  CSR of the same lists (used beyond the fourth connection) */
    const int32_t* succ_idx;
    const double* succ_len;
    const int32_t* pred_ptr;
    const int32_t* pred_idx;
    const double* pred_len;
    const double* edges;              /* (M,5) x0, y0, unit direction, length */
    const int32_t* edge_ix;           /* (M,2) node pair */
    const int32_t* cell_ptr;          /* (gnx*gny+1) */
    const int32_t* cell_edges;
    int32_t N, M, gnx, gny;
    double gx0, gy0, gcell;
} StrivePlannerMap;

/* PlannerConfig of the reference (:25-59) + two derived values evaluated on the host with numpy's arithmetic. */
typedef struct StrivePlannerCfg {
    double dt, preddt, xydistmax, smax, accmax, interacdist, col_plim, score_wmin, score_wfac;
    double cdistmax;                  /* 1 - cos(radians(cdistang)) */
    double tmax;                      /* nsteps * preddt */
    double predsfacs[4], predafacs[4], planaccfacs[4];
    int32_t nsteps, npredsfacs, npredafacs, nplanaccfacs, plannspeeds;
} StrivePlannerCfg;

/* The planner after reset() (:109-127): initial world of every scene, scene-sorted, the ego at position `ego_idx` of
 * its scene.  init (NO,6) = x, y, heading angle, signed speed, length, width.  Rows of `agent_obs` (the non-ego objects
 * in scene order) are described by row_obj (index into init) and row_scene. */
typedef struct StrivePlanner {
    StrivePlannerCfg cfg;
    int32_t nmaps;
    StrivePlannerMap maps[STRIVE_PLANNER_MAXMAPS];
    int32_t B, NO, NR, ego_idx;
    const int32_t* ptr;               /* (B+1) object offsets */
    const int32_t* scene_map;         /* (B) map of each scene */
    const double* init;               /* (NO,6) */
    const int32_t* row_obj;           /* (NR) */
    const int32_t* row_scene;         /* (NR) */
} StrivePlanner;

/* nstep = int(planner_t[-1] / dt) planner steps after the initial one; traj_cap = predicted trajectories kept per scene
 * and planner step (other objects x routes x speed profiles). */
size_t strive_planner_workspace_bytes(const StrivePlanner* pl, int32_t nstep, int32_t traj_cap);

/* HardcodeNuscPlanner.rollout(agent_obs, agent_t, agent_ptr, planner_t) (:178-276) for all scenes: agent_obs (NR,T,4)
 * fp32 UNNORMALISED (x, y, cos, sin) futures of the non-ego objects (NaN from the first unobserved frame on), agent_t (T),
 * t_out (nstep+1) = linspace(dt, dt*nstep, nstep+1) and planner_t (TP) float64 -> plan (B,TP,4) float64.
 * Per planner step: lane matching / clustering / breadth-first route enumeration / blended arc-length routes for every
 * object (compute_splines, :559-598), 5-circle gaps between the ego's candidate speed profiles and every predicted
 * trajectory (compute_action, :829-857), world update (update_wstate, :601-621).
 * status (B, STRIVE_PLANNER_NSTATUS) int32 on the device, zeroed by the caller once and then only ever SET by the kernels
 * (sticky over rollouts): a non-zero entry of row b names a capacity or range violation in scene b (0 matches, 1 clusters,
 * 2 chains, 3 chain nodes, 4 knots, 5 route range, 6 trajectory cap, 7 action check) -- the cases in which the reference's
 * numpy planner raises (interp1d bounds, :411-428; the speed assertion, :659-666), which there ends the run of that scene
 * (adv_scenario_gen.py:540-543 with the shipped batch_size 1).  The plan of an affected scene is NaN; every other scene of
 * the batch is planned as if the failing one were not there (scenes share nothing but this call).
 * alive (B) uint8 or NULL: written last, alive[b] = (row b of status is all zero) -- the device-side mask the closed loop
 * hands to strive_adv_gen_fwd (StriveAdvGen.scene_alive) so that a failed scene leaves the losses without a host round trip. */
int strive_planner_rollout(const StrivePlanner* pl, const double* agent_obs, const double* agent_t, int32_t T,
                           const double* t_out, int32_t nstep, const double* planner_t, int32_t TP, int32_t traj_cap,
                           double* plan, int32_t* status, uint8_t* alive, void* ws, size_t ws_bytes, strive_stream_t stream);

/* Debug view used by the parity tests: routes of one object pose (x, y, h, s) on map `mapix` as the planner builds them.
 * Outputs: nroutes (1), nk (maxr) knots per route, knots (maxr, maxk, 5) = s, x, y, cos, sin. */
int strive_planner_routes(const StrivePlanner* pl, int32_t mapix, const double* pose4, int32_t maxr, int32_t maxk,
                          int32_t* nroutes, int32_t* nk, double* knots, int32_t* status, strive_stream_t stream);

/* Debug view used by the parity tests: where strive_planner_rollout keeps its tables in the caller's workspace (host only, no
 * launch).  After a rollout the workspace holds, for ALL planner steps, the other objects' states and presence (update_wstate,
 * reference src/planners/hardcode_goalcond_nusc.py:601-621), their predicted trajectories and counts (:686-721) and the ego's
 * poses; and, for the LAST planner step, the ego's route, its stop preference, the speed profiles (gen_sprofiles, :804-826),
 * their circle centres (:860-882) and the partial gap minima and near-trajectory counts per chunk (:885-897).
 * out (n_out >= STRIVE_PLANNER_NLAYOUT) int64: byte offsets of  0 wstate (NR,K,4) f64, 1 present (NR,K) i8,
 * 2 traj (B*K,cap,ENT) f64 [object x, y, l, w, duplicate mask, NT x (x, y, h)], 3 traj_cnt (B*K) i32, 4 scene_bad (B) i32,
 * 5 route_nk (B) i32, 6 prefer_stop (B) i32, 7 part_cnt (B,NCHUNK) i32, 8 ego (B,8) f64, 9 route (B,5,MAXK) f64,
 * 10 prof (B,MAXPROF,3) f64 [s1, acc, final distance], 11 circ (B,P,NT,10) f64, 12 part (B,NCHUNK,P,NT) f64,
 * 13 poses (B,K,4) f64; then 14 the bytes carved, 15 K, 16 cap, 17 ENT, 18 P, 19 NT, 20 nchunk (the chunks per scene the rollout
 * launches, of which NCHUNK is the stride), 21 MAXK, 22 MAXPROF, 23 NCHUNK. */
#define STRIVE_PLANNER_NLAYOUT 24
int strive_planner_workspace_layout(const StrivePlanner* pl, int32_t nstep, int32_t traj_cap, int64_t* out, int32_t n_out);

/* Operator-level views of two building blocks the rollout kernels evaluate in registers (the kernels call the same device
 * functions); used by the parity tests against the reference's own outputs.
 *
 * strive_bicycle_step: TrafficModel.sim_traj -> car_dynamics for one step (reference src/models/traffic_model.py:645-650,
 * 714-733, src/models/common.py:47-68, src/utils/transforms.py:8-29) with dec's normaliser statistics and bicycle
 * parameters: state (N,6) normalised, dec_out (N,2) the decoder's (acceleration, yaw acceleration) output, lw0 (N) the
 * normalised vehicle length -> out (N,6) normalised next state; with g_out (N,6) also the adjoints g_state (N,6) and
 * g_dec (N,2) (zero through an active clamp).
 * strive_rel_pose: transform2frame(frame, poses) (reference src/utils/transforms.py:78-139, forward branch): frame (N,4),
 * poses (N,M,4) -> out (N,M,4); with g_out also g_frame (N,4) (summed over M) and g_poses (N,M,4). */
int strive_bicycle_step(const StriveDecoder* dec, const float* state, const float* dec_out, const float* lw0, const float* g_out,
                        float* out, float* g_state, float* g_dec, int32_t N, strive_stream_t stream);
int strive_rel_pose(const float* frame, const float* poses, const float* g_out, float* out, float* g_frame, float* g_poses,
                    int32_t N, int32_t M, strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Scene dataset: the part of the reference's NuScenesDataset that follows the devkit (reference
 * src/datasets/nuscenes_dataset.py:416-589 post_process, :594-704 __getitem__, plus the PyG DataLoader collation), on
 * tables that stay on the device.  All scenes are flattened: a scene's agents are consecutive, the ego first; an agent's
 * table rows are the frames of its scene's timeline.
 * ---------------------------------------------------------------------------------------------- */

/* The records compile_data hands to post_process (reference src/datasets/nuscenes_dataset.py:350-414), nothing derived. */
typedef struct StriveTracks {
    int32_t S, A, O;                  /* scenes, agents (egos included), observations */
    const int32_t* frame_ptr;         /* (S+1) into ego_t */
    const int64_t* ego_t;             /* microseconds: a scene's timeline */
    const int32_t* agent_ptr;         /* (S+1); a scene's first agent is its ego */
    const int32_t* scene_map;         /* (S) map index */
    const int32_t* agent_scene;       /* (A) */
    const int32_t* use;               /* (A) 0: the agent's category is not asked for (it is dropped) */
    const double* lw;                 /* (A,2) length, width */
    const int32_t* obs_ptr;           /* (A+1) */
    const int32_t* obs_frame;         /* (O) index on the scene's timeline (ego_t_map, :435) */
    const double* obs;                /* (O,5) x, y, h, hcos, hsin */
} StriveTracks;

/* scene2info of every scene (:463-571) as flat float64 tables; scenario scenes (compile_scenarios, :231-290) follow the
 * track scenes in the same tables. */
typedef struct StriveSceneTables {
    int32_t S, A;
    int64_t R;                        /* table rows: sum over agents of the frames of their scene */
    const int32_t* agent_ptr;         /* (S+1) */
    const int32_t* scene_T;           /* (S) frames */
    const int32_t* scene_map;         /* (S) */
    const int64_t* row_ptr;           /* (A) first row of each agent */
    const int32_t* cat;               /* (A) column of the one-hot `sem`; the ego's is that of 'car' (:613) */
    const double* lw;                 /* (A,2) */
    double* traj;                     /* (R,6) x, y, hcos, hsin, s, hdot */
    double* accel;                    /* (R,2) |d vel|, ddh */
    int32_t* is_vis;                  /* (R) */
    int32_t* kept;                    /* (A) 0: never on the drivable layer (:532-534) or not asked for */
} StriveSceneTables;

typedef struct StriveNorm {
    float state_mean[6], state_std[6], att_mean[2], att_std[2];
} StriveNorm;

/* post_process for all agents of all track scenes in one launch (one workgroup per agent), float64, every operation
 * rounded on its own.  Per observation of a non-ego agent: check_on_layer (reference src/datasets/nuscenes_utils.py:266-298
 * with gen_car_coords :205-232) on raster layer 0 and, with carpark_layer > 0 (a raster that has a car-park layer), on that layer: grid L = rint(l / mdx),
 * W = rint(w / mdx) (mdx = mean of all dx), torch.linspace(-1, 1, n) in fp32 widened (lin holds the tables of n = 0..nmax
 * back to back, table n at lin_off[n]), scaled by l/2 and w/2, rotated, translated, divided by the map's dx, rounded half
 * to even, outside pixels read pixel (0,0); a frame is kept if drivable >= 0.3 and carpark < 0.3 (fractions in fp32,
 * :513-522).  Kept observations are scattered on the scene timeline (:524-530); velocity and heading_change_rate
 * (nuscenes_utils.py:134-199: backward differences, forward at frame 0 and at a frame that follows a NaN unless it is the
 * last) give s, |d vel|, hdot, ddh; frames with NaN speed lose their position (:545-551).  The ego takes the same
 * arithmetic without the filter (:433-453).  Writes traj, accel, is_vis, kept of the first tr->A agents of tb.
 * ws: tb->R * 8 doubles. */
int strive_dataset_post_process(const StriveTracks* tr, const StriveMap* map, const StriveSceneTables* tb, int32_t carpark_layer,
                                double mdx, const int32_t* lin_off, const float* lin, int32_t nmax, void* ws, size_t ws_bytes,
                                strive_stream_t stream);

/* seq (N,2) = (scene, first frame) of every window; counts[i] = agents __getitem__ would return for window i (:630-649):
 * the ego, and every kept agent without a NaN in traj[midx-1] and, with require_full_past, in traj[:midx]. */
int strive_dataset_window_counts(const StriveSceneTables* tb, const int32_t* seq, int32_t N, int32_t npast, int32_t nfuture,
                                 int32_t require_full_past, int32_t* counts, strive_stream_t stream);

/* __getitem__ (:594-704) and the DataLoader collation of B windows in one launch, one workgroup per window.
 * meta (3, B+1) int64 from the host, which knows the counts: window indices, node offsets `ptr`, edge offsets.  The
 * selected agents are compacted in table order (ego first); float64 -> fp32, then (x - mean) / std in fp32 (:651-663).
 * past, past_gt (NA,PT,6), future, future_gt (NA,FT,6), lw (NA,2), sem (NA,NC), past_vis (NA,PT), future_vis (NA,FT) fp32;
 * batch (NA), map_idx (B), edge_index (2,E) int64: per window the source-major clique without self loops (:678-687),
 * offset by its first node. */
int strive_dataset_gather_batch(const StriveSceneTables* tb, const int32_t* seq, const int64_t* meta, int32_t B, int32_t npast,
                                int32_t nfuture, int32_t NC, int32_t require_full_past, const StriveNorm* norm, float* past,
                                float* past_gt, float* future, float* future_gt, float* lw, float* sem, float* past_vis,
                                float* future_vis, int64_t* batch, int64_t* map_idx, int64_t* edge_index, int64_t E,
                                strive_stream_t stream);

/* One Adam step of the training loop (reference src/train_traffic.py:275-277 creates optim.Adam(model.parameters(), lr,
 * weight_decay), :113-115 steps it) over ALL parameters at once, in one kernel launch: p, g, m (exp_avg), v (exp_avg_sq) are flat
 * fp32 arrays of n elements, 16-byte aligned -- the unpadded concatenation of the parameter tensors in model.parameters() order.
 * Per element, in fp32, the arithmetic of torch.optim.Adam's single-tensor form (amsgrad and maximize off):
 *   g' = g + weight_decay p;  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g' g';
 *   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * with bc1 = 1 - beta1^t and bc2 = 1 - beta2^t formed by the host in double.  p, m, v are updated in place, g is only read.
 * seg_off (nseg + 1 int64 on the device, seg_off[0] = 0 <= ... <= seg_off[nseg] = n) names the tensors; if seg_absmax != NULL the
 * same pass writes seg_absmax[s] = max |p_new| over segment s (nseg floats; 0 for an empty segment, NaN if the segment holds a NaN):
 * exact and independent of the order of execution (an integer maximum of the bit patterns).  The table need not be cleared by the
 * caller.  seg_off and nseg are ignored when seg_absmax is NULL. */
int strive_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                     double weight_decay, double bc1, double bc2, const int64_t* seg_off, int32_t nseg, float* seg_absmax,
                     strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Scenario pictures
 * ---------------------------------------------------------------------------------------------- */

/* F pictures of a map crop with cars, trajectories and markers in one launch, no host synchronisation: what the reference draws
 * with one matplotlib figure per picture (reference src/datasets/nuscenes_utils.py:655-702 viz_map_crop, :717-731
 * render_map_observation, :733-835 render_obj_observation, :837-853 plot_box / plot_car; called from reference
 * src/viz_scenario_dir.py:53-107 and reference src/eval_adv_gen.py:537-640).  out: (F, L, L, 3) uint8 RGB, row 0 at the top.
 *
 * Frame: the crop's pixel frame of objs2crop (reference src/datasets/map_env.py:231-254): x along the crop's first axis, y along
 * its second, y up.  Pixel (row, col) is the square [col, col + 1] x [L - 1 - row, L - row].  matplotlib's half-pixel offset
 * between imshow's pixel centres and xlim(0, L) is NOT reproduced.  Only square pictures: W must equal L (the reference's xlim /
 * ylim mix the axes otherwise); anything else is an error.
 *
 * Background: white, then the map's layers in channel order, c += (v_i alpha_i)(col_i - c) with v_i the raster byte that
 * get_map_crop_pos(pose, mapix, bounds, L, L) holds at [i, col, L - 1 - row] (imshow(x[i].T, origin='lower')); the gather is the
 * crop's, bit for bit, the crop itself is not materialised.  The bounds enter as the crop's own fp32 tables: lin (NB, 2, L) holds
 * torch.linspace(b[0], b[2], L) then torch.linspace(b[1], b[3], L) for NB sets of bounds, lin_ix (F) picks a picture's set.
 * layer_rgb / layer_alpha: the reference's colour list (darkgray, coral, orange, gold, lightblue, lightblue; 1, .6, .6, .6, 1, .5);
 * a map of more than STRIVE_RENDER_MAX_LAYERS layers is an error.  no_map[f] != 0: white background.
 *
 * Primitives: picture f draws prims[prim_range[2f] .. prim_range[2f+1]) in table order.  A record is STRIVE_RENDER_PRIM_FLOATS
 * fp32 words (the table 16-byte aligned):
 *   [0] kind (int32 bits)   [1] cx  [2] cy   [3] hx  [4] hy   [5] l (car) or diameter (disc)  [6] w
 *   [7..9] RGB in [0, 1]   [10] alpha   [11] stroke width: the car's outline, the polyline   [12] stroke width of the car's heading
 *   [13] [14] vertex range [begin, end) into verts (NV, 2) (int32 bits, polyline)   [15] unused
 * THE COVERAGE RULE IS THIS LIBRARY'S OWN (as strive_map_rasterize's is; Agg's anti-aliasing is not reproduced): coverage of a
 * shape on a pixel = the number of the 4 x 4 regular sub-samples at offsets (k + 1/2)/4 that lie in the shape (boundary included)
 * / 16; blend c += (alpha cov)(col - c) in fp32; stored byte rint(255 c), clamped.  No atomics; a pixel's bytes depend only on
 * its own picture's inputs.
 *   car       with (u, v) the sub-sample in the car's frame (heading normalised; zero heading = (1, 0)): fill |u| <= l/2 and
 *             |v| <= w/2 in RGB; outline in black, |u| <= l/2 + e and |v| <= w/2 + e and not (|u| < l/2 - e and |v| < w/2 - e),
 *             e = [11]/2; heading stroke in black, -h <= u <= l/2 + h and |v| <= h, h = [12]/2.  Three blends with the car's alpha.
 *   polyline  the union of the capsules of radius [11]/2 around consecutive vertices (round caps and joins), blended ONCE.
 *   disc      distance to (cx, cy) <= [5]/2; every disc is blended on its own.
 * A primitive with a NaN in its geometry, or a polyline of fewer than 2 vertices, draws nothing. */
#define STRIVE_RENDER_MAX_LAYERS 6
#define STRIVE_RENDER_PRIM_FLOATS 16
#define STRIVE_RENDER_CAR 0
#define STRIVE_RENDER_POLYLINE 1
#define STRIVE_RENDER_DISC 2
typedef struct StriveRenderJob {
    const float* pose;            /* (F, 4) crop pose x, y, hx, hy (unnormalised) */
    const int32_t* mapix;         /* (F) */
    const float* lin;             /* (NB, 2, L) */
    const int32_t* lin_ix;        /* (F) */
    const int32_t* prim_range;    /* (F, 2) */
    const int32_t* no_map;        /* (F) */
    const float* prims;           /* (NP, STRIVE_RENDER_PRIM_FLOATS) */
    const float* verts;           /* (NV, 2) */
    int32_t F, L, W, NP, NV, reserved;
    float layer_rgb[STRIVE_RENDER_MAX_LAYERS * 3];
    float layer_alpha[STRIVE_RENDER_MAX_LAYERS];
} StriveRenderJob;

int strive_render_pictures(const StriveMap* map, const StriveRenderJob* job, uint8_t* out, strive_stream_t stream);

/* The tables strive_render_pictures reads (pose, mapix, prim_range, prims, verts), built on the device from a batch that lives
 * there, for any number of VIEWS in one launch and without a host synchronisation: what the reference's viz_scene_graph
 * (reference src/datasets/nuscenes_utils.py:477-621) hands to viz_map_crop / viz_map_crop_video (:632-653), followed by the
 * artists render_obj_observation (:733-835) makes of it.  One workgroup per picture (grid-stride), no atomics, ordinary stores;
 * in-picture offsets by a workgroup scan.  The bytes a picture's slots receive depend on its own scene and view only.
 *
 * Inputs, all NORMALISED and only read: past_gt (NA, PT, past_stride >= 4), future_gt (NA, FT, future_stride >= 4), lw (NA, 2),
 * ow_gt (NA, FT, 4) or NULL, up to STRIVE_SCENE_DRAW_PREDS prediction sets pred[i] (NA, pred_NS[i], pred_FPT[i], 4);
 * scene_ptr (B + 1) agent offsets; map_idx (B) int64.  DEVIATION: the reference unnormalises the caller's graph in place and
 * normalises it back, which changes last bits of the caller's batch; here every value is unnormalised in registers with
 * MeanStdNormalizer.unnormalize's two fp32 operations (one rounded multiply, one rounded add) and the batch is never written.
 *
 * A view = one viz_scene_graph call's picture set, an int32 record of STRIVE_SCENE_DRAW_VIEW_INTS:
 *   [0] bidx   [1] flags (below)   [2] [3] first drawn agent (scene-local) and count: (0, n), or (aidx, 1)
 *   [4] [5] first ground-truth agent and count (0: no ground-truth pass): show_gt / show_gt_idx / aidx resolved by the host
 *   [6] crop_t   [7] prediction set, -1: future_gt is drawn (NS = 1)   [8] first row of this view's marker colours in `rainbow`
 *   [9] first row of its styles in `style`, -1: the defaults   [10..15] unused
 * and a float record view_f (4): bounds[0], bounds[1], L / (bounds[2] - bounds[0]), W / (bounds[3] - bounds[1]) (host doubles,
 * rounded to fp32 as numpy does for objs2crop).  QUIRK KEPT: with aidx the reference slices crop_objs but neither crop_lw nor
 * the colours, so the drawn agent takes row 0's size, colour and style: sizes and styles are indexed by the POSITION in the
 * drawn list, trajectories by the agent.
 *
 * A picture = an int32 record of STRIVE_SCENE_DRAW_PIC_INTS: [0] view  [1] sample s, -1: the overview (all samples, all steps)
 * [2] step t (frame (s, t) of viz_map_crop_video holds car_kin[:, s:s+1, t:t+1], T = 1, no ground-truth pass)
 * [3] first primitive slot  [4] first vertex slot  [5] primitive capacity  [6] vertex capacity  [7] unused.
 * Capacities come from shapes, on the host; NaNs only shrink a picture's count; prim_range[f] = [slot, slot + count).
 *
 * Crop pose (x, y, hx, hy), unnormalised: past_gt[first agent of the scene, PT - 1]; with STRIVE_SCENE_DRAW_CROP_T the same
 * agent's row crop_t of past_gt (crop_t < PT) or future_gt; with STRIVE_SCENE_DRAW_CENTER ((mx, my), 1, 0), (mx, my) the mean
 * over the scene's agents n, samples s and steps t (past, repeated per sample, then the drawn future) of every position without
 * a NaN: partial sums in float64, thread i of 256 taking items i, i + 256, ... of the (n, s, t) order, then a fixed binary tree;
 * divided in float64, rounded once.  It depends on nothing outside the scene.
 *
 * Frame: objs2crop (reference src/datasets/map_env.py:231-254 with objects2frame) in fp32, unfused: theta = atan2(hy_c, hx_c);
 * (x', y') = ((x - x_c) cos + (y - y_c) sin, (y - y_c) cos - (x - x_c) sin); heading (cos, sin)(atan2(hy, hx) - theta);
 * x' = (x' - b0) sl, y' = (y' - b1) sw; sizes l sl, w sw.
 *
 * Records, in matplotlib's draw order: discs (markers, z 1), polylines (z 2), cars (z 3); inside a group the ground-truth pass
 * (white lines and cars, alpha 0.7, width 1, size 8, no initial car) before the prediction pass; inside a pass agents, then
 * samples, then steps.  A step with a NaN in its four crop values is left out BEFORE vertices and markers are emitted, so a line
 * joins across a gap; a trajectory without a step gives no line.  With STRIVE_SCENE_DRAW_TRAJ: one disc per step in
 * rainbow[row + t] (the host's gist_rainbow(linspace(0, 1, T)); T = PT + FT for the ground truth at rb_gt_off, T = 1 for a frame
 * at rb_one_off), diameter (sqrt(size) + 1) k; one polyline per trajectory, width linewidth k, its vertices the discs' centres;
 * one car per drawn agent at the first step of sample 0 (of the frame's sample) whose crop x is not NaN -- an agent without one
 * sets STRIVE_SCENE_DRAW_NO_STEP (the reference raises IndexError, :801, :810) and gets no car.  Without it: one car per step
 * without a NaN, alpha = the agent's at t = 0 and 0.1 + (1 - t / T) 0.2 after, evaluated in float64 and rounded once.  Styles:
 * style (rows, 8) fp32 r, g, b, alpha, line width, marker size, 2 unused; default colour cycle_rgb[position % 9], 0.7, 1.0, 8.0.
 * k (float64): picture pixels per point; products with k are formed in float64 and rounded once, as the host path's.
 *
 * status (F) int32 per picture (one word per picture, not per view: pictures of a view are written by different workgroups
 * and nothing is atomic; the host ORs them): bits below, and with NO_STEP (position of the first such agent + 1) << 8.  A
 * picture with BAD_VIEW (a record that does not fit the shapes) gets an empty range and a NaN pose. */
#define STRIVE_SCENE_DRAW_PREDS 4
#define STRIVE_SCENE_DRAW_VIEW_INTS 16
#define STRIVE_SCENE_DRAW_PIC_INTS 8
#define STRIVE_SCENE_DRAW_TRAJ 1          /* viz_traj */
#define STRIVE_SCENE_DRAW_CENTER 2        /* center_viz */
#define STRIVE_SCENE_DRAW_CROP_T 4        /* crop_t given */
#define STRIVE_SCENE_DRAW_OW_GT 8         /* the ground-truth pass draws ow_gt */
#define STRIVE_SCENE_DRAW_BAD_MAP 1       /* map_idx[bidx] outside [0, M) */
#define STRIVE_SCENE_DRAW_NO_STEP 2       /* an agent with no observed step where the reference raises IndexError */
#define STRIVE_SCENE_DRAW_BAD_CROP_T 4    /* crop_t outside [0, PT + FT) */
#define STRIVE_SCENE_DRAW_BAD_VIEW 8      /* a view or picture record that does not fit the shapes */
typedef struct StriveSceneDraw {
    const float* past_gt;
    const float* future_gt;
    const float* lw;
    const float* ow_gt;
    const float* pred[STRIVE_SCENE_DRAW_PREDS];
    const int32_t* scene_ptr;     /* (B + 1) */
    const int64_t* map_idx;       /* (B) */
    const int32_t* views;         /* (NVIEW, STRIVE_SCENE_DRAW_VIEW_INTS) */
    const float* view_f;          /* (NVIEW, 4) */
    const int32_t* pictures;      /* (F, STRIVE_SCENE_DRAW_PIC_INTS) */
    const float* style;           /* (style_rows, 8) or NULL */
    const float* rainbow;         /* (rb_rows, 3) */
    float* pose;                  /* out (F, 4) */
    int32_t* mapix;               /* out (F) */
    int32_t* prim_range;          /* out (F, 2) */
    float* prims;                 /* out (NP, STRIVE_RENDER_PRIM_FLOATS), 16-byte aligned */
    float* verts;                 /* out (NV, 2) */
    int32_t* status;              /* out (F) */
    double k;
    int32_t NA, B, M, PT, FT, past_stride, future_stride, NVIEW, F, NP, NV;
    int32_t rb_rows, rb_gt_off, rb_one_off, style_rows;
    int32_t pred_NS[STRIVE_SCENE_DRAW_PREDS], pred_FPT[STRIVE_SCENE_DRAW_PREDS];
    float edge_px, heading_px;
    float cycle_rgb[27];
    StriveNorm norm;
} StriveSceneDraw;

int strive_scene_draw_tables(const StriveSceneDraw* job, strive_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Lane graphs built on the device (reference src/datasets/nuscenes_utils.py:28-122: remove_duplicates, process_lanegraph,
 * process_edges; the Singapore flip of src/datasets/map_env.py:131-144) and the planner's tables of them (StrivePlannerMap).
 * Input: one map's discretised lanes, in the order nmap.lane + nmap.lane_connector, before any cleaning, and per lane the
 * `outgoing` / `incoming` lists of nmap.connectivity as lane indices (-1: a token that has no lane).  float64, no contraction.
 *
 * THE LENGTH RULE, used for every distance of these entry points (duplicate test, trimming test, edge table, connection
 * lengths):   |(dx, dy)| = sqrt(fma(dy, dy, dx * dx)).   It is what numpy's np.linalg.norm of a 1-D pair evaluates (BLAS ddot
 * accumulates with a fused multiply-add); chosen over the unfused sqrt(dx*dx + dy*dy) because it agrees with every edge length
 * of the reference fixture tests/golden/g25_lane_graph.npz (804 of 804), the unfused sum with 751 of them.
 *
 * Rules, in the reference's order:
 *  1. point i < n-1 of a lane is kept iff |p[i+1] - p[i]| > eps; the last point always;
 *  2. per lane, for each outgoing lane in list order: if |succ.first - this.last| <= eps, this lane loses its last point (the
 *     next comparison uses the new last point);
 *  3. nodes are numbered in lane order.  out list of a node: the next node of its lane, or, on the lane's last node, the first
 *     nodes of its outgoing lanes in list order.  in list: the previous node, or, on the first node, the last nodes of its
 *     incoming lanes in list order;
 *  4. edges in node order, then list order: (x0, y0, dx/d, dy/d, d) and (v0, v1);
 *  5. with `flip`: xy.y = height - y, edges.y0 = height - y0, edges.dy/d *= -1 (after the edges exist);
 *  6. connection lengths (StriveLaneNode.len, *_len) from the FINAL positions.
 * Refusals (the reference's four assertions) are reported in the count record, never by a partly built table.
 *
 * Protocol: the count entry point leaves everything but the output tables in the workspace and writes counts[8] (device):
 * N, M (out connections = edges), MI (in connections), status, offending lane (rules 1, 2) or node (rules 3, 4), the lane of
 * that node, 0, 0.  The host reads that record back ONCE, allocates, and calls the fill entry point with the same input and
 * workspace; nothing is read back after the fill.  Results do not depend on the launch geometry.
 * ---------------------------------------------------------------------------------------------- */
#define STRIVE_LANE_GRAPH_OK 0
#define STRIVE_LANE_GRAPH_FIRST_POINT_DROPPED 1   /* rule 1 drops a lane's first point (remove_duplicates' assert kept[0]) */
#define STRIVE_LANE_GRAPH_LANE_EMPTIED 2          /* rule 2 leaves a lane without a point */
#define STRIVE_LANE_GRAPH_SHORT_EDGE 3            /* an edge is not longer than eps */
#define STRIVE_LANE_GRAPH_EDGE_TWICE 4            /* the same (v0, v1) appears twice */

typedef struct StriveLaneGraphIn {
    const double* pts;            /* (P, 2) every lane's points, lane after lane */
    const int32_t* lane_ptr;      /* (NL+1) */
    const int32_t* out_ptr;       /* (NL+1) CSR of the outgoing lists */
    const int32_t* out_idx;       /* lane index or -1 */
    const int32_t* in_ptr;        /* (NL+1) CSR of the incoming lists */
    const int32_t* in_idx;
    int32_t NL, P, flip, reserved;
    double eps, height;
} StriveLaneGraphIn;

typedef struct StriveLaneGraphOut {
    double* xy;                   /* (N, 2) */
    StriveLaneNode* succ;         /* (N) */
    StriveLaneNode* pred;         /* (N) */
    int32_t* succ_ptr;            /* (N+1) */
    int32_t* succ_idx;            /* (M) */
    double* succ_len;             /* (M) */
    int32_t* pred_ptr;            /* (N+1) */
    int32_t* pred_idx;            /* (MI) */
    double* pred_len;             /* (MI) */
    double* edges;                /* (M, 5) */
    int32_t* edge_ix;             /* (M, 2) */
    int32_t N, M, MI, reserved;
} StriveLaneGraphOut;

size_t strive_lane_graph_workspace_bytes(int32_t NL, int32_t P);
int strive_lane_graph_count(const StriveLaneGraphIn* in, void* ws, size_t ws_bytes, int32_t* counts, strive_stream_t stream);
int strive_lane_graph_fill(const StriveLaneGraphIn* in, void* ws, size_t ws_bytes, const StriveLaneGraphOut* out, strive_stream_t stream);

/* Uniform grid over directed edges (x0, y0, unit direction, length) -- StrivePlannerMap's cell_ptr / cell_edges, bit for bit
 * what the host's edge_grid of strive_amd/planners/hardcode_goalcond_nusc.py builds for get_lane_matches
 * (reference src/planners/hardcode_goalcond_nusc.py:298-322): p1 = p0 + len*dir (a multiply, then an add), boxes grown by
 * pad = margin*(1+1e-9) + 1e-6, origin = floor of the minima, cell ranges by floor, every edge listed in every cell its box
 * touches, ascending by edge id.  The count entry point writes *rec (device); the host reads it back ONCE and passes a host
 * copy to the fill entry point with cell_ptr (gnx*gny+1) and cell_edges (total).  The fill's workspace is sized for the cells. */
typedef struct StriveEdgeGridRec {
    double gx0, gy0;
    int64_t total;
    int32_t gnx, gny;             /* 0: the edges do not span a finite grid */
} StriveEdgeGridRec;

size_t strive_edge_grid_workspace_bytes(int32_t M, int64_t ncell);
int strive_edge_grid_count(const double* edges, int32_t M, double margin, double cell, void* ws, size_t ws_bytes, StriveEdgeGridRec* rec,
                           strive_stream_t stream);
int strive_edge_grid_fill(const double* edges, int32_t M, double margin, double cell, const StriveEdgeGridRec* rec_host, void* ws,
                          size_t ws_bytes, int32_t* cell_ptr, int32_t* cell_edges, strive_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* STRIVE_HIP_H */
