/* libsuo_hip.so -- C ABI of the MI355X-native (gfx950) hot path of rpng/suo_slam.
 *
 * Drop-in boundary.  Today the reference reaches its native code through
 * two pybind11 modules imported at /root/reference/lib/object_slam.py:9-10:
 *     lambdatwist.pnp(xs, ys, threshold)     thirdparty/lambdatwist/pnp_python_binding.cpp:57-62
 *     g2o.* graph API used by optimize()     lib/object_slam.py:703-903 (python/types/object_slam/types_object_slam.h:17-52)
 * and runs its network as stock PyTorch ops (PkpNet.forward, lib/models/pkpnet.py:80-119).
 * This header is what a ctypes / pybind stub binds instead (INTEGRATION.md shows the stubs).
 *
 * Conventions: plain C, caller-owned buffers, no exceptions; every function returns 0 on success
 * or a SUO_ERR_* code (suo_last_error() gives the message).  Pointers named *_dev are device (HBM)
 * pointers; `stream` is a hipStream_t passed as void* (NULL = internal stream + blocking).
 * All work is stream-ordered; the library never reads or writes host memory behind *_dev names.
 *
 * Runtime switches.  The library reads THIRTEEN environment variables that select between forms whose results the test suite holds against each other
 * (csrc/tune.h: env_switch), and one path -- SUO_RCCL_LIB, the RCCL library of suo_ba_comm_create_rccl when the process holds none yet; nothing else in the
 * environment changes what it does:
 *     SUO_WINO_BF16X3=0      networks are built on the fp32 matrix pipe (SUO_PIPE_F32)                      read when a network is created
 *     SUO_F16X2=0            networks are built on three bf16 terms per operand (SUO_PIPE_BF16X3)             read when a network is created
 *     SUO_STEM_X3=0          prior-less pass: RoIAlign and the stem as two launches instead of the fused one  first use, per process
 *     SUO_FUSE_UPSAMPLE=0    Hourglass up-sample add as its own launch instead of the fused tail's epilogue   first use, per process
 *     SUO_FUSE_POOL=0        2x2 max-pool as its own launch instead of the producing GEMM's epilogue          first use, per process
 *     SUO_NET_SIDE_STREAMS=n the Hourglass up1 branches on n side streams (default 0)                          first use, per process
 *     SUO_SERIAL             (set) one stream, kernels back to back: per-kernel profiling                      per call
 *     SUO_LM_CAM2=0          camera tracking on lm_cam_kernel instead of lm_cam2_kernel                        first use, per process
 *     SUO_WINO_W8=0          small launches keep the four-wave Winograd kernels (see suo_conv3x3_wino_f16x2*)  when a launch is issued: in a network,
 *                            when the graph of a crop count is captured (suo_net_prepare / first call), not at its replays
 *     SUO_WINO_HALO_DMA=0    the four-wave fp16 Winograd kernels stage their halo through registers instead of    as SUO_WINO_W8: when a launch is issued; fixed
 *                            by LDS-DMA (csrc/conv_wino_x3.hip: DMA; the two paths agree bit for bit)             in a network's graph when it is captured
 *     SUO_WINO_SKIP_DMA=0    the LDS-DMA form's fused tail with the up-sampled addend loads its skip rows into       as SUO_WINO_HALO_DMA (without which there is
 *                            registers instead of by LDS-DMA (csrc/conv_wino_x3_skip_dma.hip; bit for bit the same)  no such form)
 *     SUO_WINO_TAIL_ONE_PASS=0 the LDS-DMA form's fused tail with the next block's conv1 runs its 1x1 stages in two     as SUO_WINO_HALO_DMA (without which there is
 *                            passes of 64 pixels instead of one pass over the 128-pixel tile                         no such form)
 *                            (csrc/conv_wino_x3_one_pass.hip; bit for bit the same)
 *     SUO_GEMM_WAVES_1X4=0   the fp16 1x1 GEMMs on 128 x 128 tiles and the lin -> head chain's first stage keep their four  as SUO_WINO_W8: when a launch is issued; fixed
 *                            waves as 2 x 2 instead of side by side, each weight fragment requested once per workgroup     in a network's graph when it is captured
 *                            (csrc/gemm_bf16x3.hip: W14; bit for bit the same)
 * The thresholds and A/B knobs behind the measurements of DESIGN.md / profiles/REJECTED.md (SUO_TUNE in csrc/tune.h: launch-size thresholds, tile choices, kernel
 * selections) are compiled to their defaults; only the variant builds of tools/build_variant.sh (-DSUO_TUNING) read them from the environment.  The host side above
 * the ABI has its own, in suo_slam_amd/: SUO_HIP_LIB (path of the library), SUO_BA_GRAPH / SUO_BA_HOST_SCHEDULE / SUO_FORCE_COLLECTIVES (ba_dist.py),
 * SUO_SLAM_STORE_SLOTS (slam_score.py), SUO_SLAM_VOTE_CHAIN (object_slam.py: 0 = the host votes between the passes of a SLAM view).
 */
#ifndef SUO_HIP_H
#define SUO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUO_NUM_KP 41     /* lib/labeling/kp_config.py:82-94 */
#define SUO_HEAT 64       /* heat-map side */
#define SUO_CROP 256      /* network input side (lib/datasets/bop.py:21) */

const char* suo_last_error(void);
int suo_version(void);
/* number of visible HIP devices; <0 on error.  The product path requires one. */
int suo_device_count(void);

/* ---- keypoint network: replaces PkpNet.forward (lib/models/pkpnet.py:80-119) -------------------- */
typedef struct suo_net suo_net;

/* Build from a reference-layout state_dict (checkpoint['model'], lib/object_slam.py:92-97):
 * n float32 host tensors, names[i] the reference key ("backbone.r1.conv1.weight", ...), shapes[i]
 * its dims.  BatchNorm is folded and weights are packed for MFMA on the host, then uploaded. */
int suo_net_create(int n, const char* const* names, const float* const* data, const int64_t* const* shapes,
                   const int* ndims, int max_crops, suo_net** out);
void suo_net_destroy(suo_net* net);
int suo_net_set_graph(suo_net* net, int enable);          /* hipGraph replay of the backbone (default on) */
/* Capture the backbone graph for L crops ahead of time (with_priors: the 48-channel staging layout of the SLAM prior pass, else
 * the image-only layout).  Graphs are otherwise captured on the first call that sees a crop count -- inside whatever that call is
 * timing; a harness feeding frames with 3..max_crops detections calls this once per count at start-up.  `stream` as in the forwards
 * the graphs will be replayed on (capture is stream-agnostic; NULL = internal). */
int suo_net_prepare(suo_net* net, int L, int with_priors, void* stream);
size_t suo_net_workspace_bytes(const suo_net* net);
/* Measurement aid (nothing is launched): the launch schedule of ONE call of L crops cut from n_frames frames of H x W pixels, walked as a dry run on the
 * network's current matrix pipe.  bytes[0..5] = ALGORITHMIC HBM bytes (every operand read once, every result written once, the weights once) of the
 * staging / stem launch, the 3x3 convolutions (+ fused Residual tails), the 1x1 GEMMs, the one-launch Residual blocks, the pool / up-sample launches,
 * decode + classifier; *n_launches = kernels of the call.  bench.py's `roofline_all.whole_call` divides their sum by the measured step time. */
int suo_net_schedule_bytes(suo_net* net, int L, int n_frames, int H, int W, int with_priors, double* bytes6, int* n_launches);

/* Matrix pipe of the network's large launches (the reference runs cuDNN's fp32 convolutions, lib/models/layers/Residual.py:20-35; all three forms are held
 * to its outputs at 1e-5, tests/test_gpu_cnn.py).  Chosen when the network is created -- SUO_WINO_BF16X3=0: SUO_PIPE_F32; SUO_F16X2=0: SUO_PIPE_BF16X3;
 * default SUO_PIPE_F16X2 -- and lowered at run time by suo_net_set_pipe (F16X2 -> BF16X3; the fp32 form only when created with it).
 *   SUO_PIPE_F32     v_mfma_f32_32x32x2_f32, exact fp32 products
 *   SUO_PIPE_BF16X3  operands as three bf16 terms, 6 of 9 cross products, fp32 accumulate (csrc/bf16x3.h): fp32's range
 *   SUO_PIPE_F16X2   operands as two fp16 terms, 3 of 4 cross products, fp32 accumulate (csrc/f16x2.h): half the matrix-pipe work, fp16's RANGE --
 *                    activations enter times 2^s (s = 4 unless calibrated, see suo_net_calibrate), so a forward in which some |activation| >= 65504 / 2^s is not
 *                    computable in this form.  The kernels detect
 *                    that (they never write inf silently) and raise a flag:
 * Validity is PER CALL: a forward's outputs are invalid if and only if its own activations left the range.  Every forward is numbered 1, 2, ... in issue order
 * (suo_net_last_call() returns the number of the last one issued); on SUO_PIPE_F16X2 it ends with a one-lane launch on its stream that moves the kernels'
 * flag into that call's word (mapped host memory) and clears it for the next call, so a later call still running cannot mark an earlier one.
 * suo_net_call_range_exceeded(net, call) returns 1 when that call left the range -- its outputs are INVALID; the network has then already been moved to
 * SUO_PIPE_BF16X3 and the caller re-issues it (and whatever it enqueued behind it that consumed its outputs) --, 0 when its outputs are valid, -1 when it
 * cannot tell (the call has not finished, or is older than the network's last 64 calls; suo_last_error() says which).  Call it after synchronising on the
 * call's outputs and before using them.  The network moves to SUO_PIPE_BF16X3 when a query reports an invalid call, not before: calls issued meanwhile
 * still run on SUO_PIPE_F16X2 and are queried like any other.
 * suo_net_range_exceeded() returns 1 when a forward since its last call left the range (whether or not suo_net_call_range_exceeded reported it) and clears
 * that record; on 1 the network has been moved to SUO_PIPE_BF16X3.  Call it after synchronising the stream.  Forwards on the NULL stream (blocking) check
 * their own call and re-issue it by themselves. */
#define SUO_PIPE_F32 0
#define SUO_PIPE_BF16X3 1
#define SUO_PIPE_F16X2 2
int suo_net_get_pipe(const suo_net* net);
int suo_net_set_pipe(suo_net* net, int pipe);
int suo_net_range_exceeded(suo_net* net);
uint64_t suo_net_last_call(const suo_net* net);
int suo_net_call_range_exceeded(suo_net* net, uint64_t call);

/* Per-site activation exponents of SUO_PIPE_F16X2 (csrc/f16x2.h).  A SITE is the input operand of one convolution that has fp16 planes, whichever kernel
 * computes it; it enters the two-term split times 2^s.  A network starts with s = 4 at every site (the fixed factor 16 above: outputs bit-identical to
 * an uncalibrated network); the image stem keeps 2^4 and is no site.  Weights whose activations reach thousands (trained checkpoints can) leave the range at
 * s = 4 and cost the network its fp16 form; calibration picks s per site from the data instead:
 *   suo_net_calibrate      one probe forward of the frames and boxes given (the inputs of suo_net_forward_frames, prior-less) on SUO_PIPE_BF16X3, every block on
 *                          its per-layer launches so each site's operand is measured whatever the crop count routes where; per site the largest s with
 *                          2^s k max|x| <= 4094 (suo_f16x2_shift_for).  The probe is not a numbered call and leaves the range record alone.  Fails, leaving the
 *                          network unchanged, when a site is unmeasured or its max is not finite.  Blocks until done (stream: where the probe runs; NULL: own).
 *   suo_net_f16x2_sites    the number of sites; suo_net_f16x2_site_name(net, i) its convolution's state-dict prefix ("backbone.Residual.3.conv2")
 *   suo_net_get_f16x2_shifts / suo_net_set_f16x2_shifts   all n sites' s (set: each in [-26, 26]) -- to store a calibration with its checkpoint, or share it
 * calibrate and set wait for the device's work in flight, then rewrite the factors in place (captured graphs stay valid).  After either succeeds a network built
 * for SUO_PIPE_F16X2 that had fallen back to SUO_PIPE_BF16X3 runs SUO_PIPE_F16X2 again (the only way up; suo_net_set_pipe only lowers).  Networks built without
 * the fp16 form have no sites: calibrate / set fail.
 * suo_f16x2_shift_for: the rule, host only -- the largest s with 2^s k amax <= 65504 / 16 (k = 4 for ksize 3: the Winograd transform's bound; k = 1 for ksize 1),
 * clamped to [-26, 26] (2^s and every 2^-(t_n + s) stay normal fp32); amax = 0 gives 4; amax negative, inf or nan, or ksize not 1 or 3: SUO_ERR_ARG. */
int suo_net_calibrate(suo_net* net, const void* imgs_dev, int img_format, int H, int W, const float* boxes_dev, const int* box_img_dev, int L, void* stream);
int suo_net_f16x2_sites(const suo_net* net);
const char* suo_net_f16x2_site_name(const suo_net* net, int i);
int suo_net_get_f16x2_shifts(const suo_net* net, int* out, int n);
int suo_net_set_f16x2_shifts(suo_net* net, const int* shifts, int n);
int suo_f16x2_shift_for(float amax, int ksize, int* out);

/* One frame: image either SUO_IMG_U8_HWC = uint8 [H,W,3] as cv2.imread gives it (scaled by 1/255 on
 * device: object_slam.py:1092 fused) or SUO_IMG_F32_CHW = float32 [3,H,W] already scaled (the tensor
 * PkpNet.forward receives); boxes float32 [L,4] xyxy pixels, priors float32 [L,41,256,256] or NULL (= zeros, pkpnet.py:95-97).
 * Outputs (device): uv [L,41,2], cov [L,41,2,2], kp_mask [L,41] (sigmoid prob), optional
 * kp_mask_logits [L,41] and prob_logits [L,41,64,64] (NCHW, the reference's ret["prob_logits"]). */
#define SUO_IMG_U8_HWC 0
#define SUO_IMG_F32_CHW 1
int suo_net_forward(suo_net* net, const void* img_dev, int img_format, int H, int W, const float* boxes_dev, int L,
                    const float* priors_dev, float* uv_dev, float* cov_dev, float* kp_mask_dev,
                    float* kp_mask_logits_dev, float* prob_logits_dev, void* stream);

/* Several independent frames in one call (they batch like crops do): imgs_dev is a contiguous stack of frames
 * [B,H,W,3] uint8 (or [B,3,H,W] float32), box_img_dev[l] the frame index of crop l; everything else as above. */
int suo_net_forward_frames(suo_net* net, const void* imgs_dev, int img_format, int H, int W, const float* boxes_dev,
                           const int* box_img_dev, int L, const float* priors_dev, float* uv_dev, float* cov_dev,
                           float* kp_mask_dev, float* kp_mask_logits_dev, float* prob_logits_dev, void* stream);

/* The SLAM pass with priors (lib/object_slam.py:486-519 -> __run_kp_model): instead of the dense prior tensor that the
 * reference renders on the host with make_prior_kp_input (lib/utils/utils.py:356-411) and uploads -- 10.7 MB per crop --
 * pass the projected keypoints themselves: prior_uv_dev float32 [L,41,2] NDC, prior_mask_dev uint8 [L,41] (0 = channel
 * stays zero; non-finite keypoints are skipped like utils.py:402).  The 91x91 Gaussian stamps are evaluated while the
 * crop is staged.  box_img_dev may be NULL (all crops from frame 0).  Everything else as suo_net_forward_frames. */
int suo_net_forward_prior_kp(suo_net* net, const void* imgs_dev, int img_format, int H, int W, const float* boxes_dev,
                             const int* box_img_dev, int L, const float* prior_uv_dev, const uint8_t* prior_mask_dev,
                             float* uv_dev, float* cov_dev, float* kp_mask_dev, float* kp_mask_logits_dev,
                             float* prob_logits_dev, void* stream);
/* make_prior_kp_input on the device: the dense [L,41,256,256] tensor the reference builds (parity / interoperability) */
int suo_render_priors(const float* prior_uv_dev, const uint8_t* prior_mask_dev, int L, float* out_dev, void* stream);

/* Backbone only (HourglassNet.forward, lib/models/hg.py:95-119): staged NHWC input [L,256,256,48]
 * (44 channels zero padded to 48; NULL = re-use the input staged by the previous call) -> logits
 * [L,41,64,64] NCHW (may be NULL).  Test / profiling entry for the conv stack. */
int suo_net_backbone(suo_net* net, const float* staged_dev, int L, float* prob_logits_dev, void* stream);

/* Frame upload (the H2D of lib/object_slam.py:1096-1098) as a stream-ordered kernel: src is PINNED host memory (hipHostMalloc /
 * torch pin_memory, i.e. mapped into the device's address space; 16-byte aligned like dst_dev), read over the host link with
 * coalesced 16-byte loads.  Use instead of hipMemcpyAsync in front of a network call: see csrc/misc.hip for the measured reason. */
int suo_upload(void* dst_dev, const void* src_pinned_host, size_t bytes, void* stream);

/* ---- stand-alone stages (each is also a parity-test entry point) --------------------------------- */
/* spatial_softmax + post_process_kp (pkpnet.py:13-63): logits [L,41,64,64] -> uv, cov, mean logit.
 * Optional outputs (NULL = skipped): argmax_idx_dev int32 [L,41] = flat index h*64+w of the first maximum of each heat-map, exactly what
 * torch.argmax(logits.flatten(2), -1) returns -- the reference decodes with a SOFT arg-max only (pkpnet.py:28-63), this diagnostic hard
 * arg-max is the bit-exact integer keypoint output; prob_dev float32 [L,41,64,64] = the soft-max itself, ret["prob"]
 * (pkpnet.py:111). */
int suo_decode_heatmaps(const float* logits_dev, int L, float* uv_dev, float* cov_dev, float* mean_logit_dev, int32_t* argmax_idx_dev,
                        float* prob_dev, void* stream);
/* classifier (pkpnet.py:74-78,116-118): sigmoid(W relu(mean_logit) + b) */
int suo_classifier(const float* mean_logit_dev, const float* w_dev, const float* b_dev, int L,
                   float* kp_logit_dev, float* kp_prob_dev, void* stream);
/* keypoint validity masks (object_slam.py:1100-1115); model_mask may be NULL (= all true) */
int suo_keypoint_masks(const float* uv_dev, const float* cov_dev, const float* kp_prob_dev, const uint8_t* model_mask_dev,
                       int L, float bbox_thresh, float kp_var_thresh, uint8_t* mask_dev, void* stream);
/* roi_align + concat (pkpnet.py:93-101) -> NHWC [L,256,256,48] (44 channels, zero padded to 48) */
int suo_roi_align_concat(const void* img_dev, int img_format, int H, int W, const float* boxes_dev, int L, const float* priors_dev,
                         float* out_dev, void* stream);

/* Weight packers (host): GEMM weight W[N][K] -> the two MFMA B-operand layouts back to back, `out` holds
 * 2*Np*Kp floats: [Kp/8][Np/32][64][4] for v_mfma_f32_32x32x2 and [Kp/16][Np/16][64][4] for v_mfma_f32_16x16x4
 * (small feature maps); conv weight W[N][C][KS][KS] -> same with K' = [chunk][ky][kx][kk]. */
int suo_pack_gemm_weight(const float* w, int N, int K, int Np, int Kp, float* out);
int suo_pack_conv_weight(const float* w, int N, int C, int KS, int Np, int Cp, int CK, float* out);

/* 1x1 convolution on NHWC pixels: out = epi(pro(A1) W1 + A2 W2 + bias (+R)); see csrc/conv.hip */
int suo_conv1x1(const float* a1_dev, int lda1, int K1, const float* pro_scale_dev, const float* pro_shift_dev,
                const float* a2_dev, int lda2, int K2, const float* wp_dev, const float* bias_dev,
                const float* r_dev, int ldr, float* out_dev, int ldo, int M, int N, int n_valid, int relu,
                int nchw_hw, void* stream);
/* ... followed by nn.MaxPool2d(2, 2) in the same launch (the stem's `pool(r1(x))`, pkpnet/hg.py; Hourglass `low1(max_pool(x))`, hg.py:41):
 * the M pixels are images of H x W (W a multiple of 64, H even, N a multiple of 128); pool_out_dev is [M/4, ldo]; out_dev may be NULL
 * when only the pooled tensor is wanted.  Bit-identical to suo_conv1x1 followed by suo_maxpool2. */
int suo_conv1x1_pool(const float* a1_dev, int lda1, int K1, const float* pro_scale_dev, const float* pro_shift_dev,
                     const float* a2_dev, int lda2, int K2, const float* wp_dev, const float* bias_dev,
                     const float* r_dev, int ldr, float* out_dev, int ldo, int M, int N, int relu, int H, int W,
                     float* pool_out_dev, void* stream);
/* The same 1x1 convolution (N = 128 or 64, K a multiple of 64 up to 512, optional BN + ReLU prologue, bias, optional ReLU) at fp32 accuracy on the
 * bf16 matrix pipe: both operands are split into three bf16 terms and 6 of the 9 cross products are accumulated in fp32
 * (csrc/gemm_bf16x3.hip; what suo_net_forward launches for conv1 of its Residual blocks at >= 4096 pixels on the fp16 pipe, >= 32768 on the bf16x3 pipe (csrc/net.hip: x3_min_rows) unless SUO_WINO_BF16X3=0).
 * wp3 = suo_pack_gemm_weight_bf16x3(W[N][K]) -> 3*N*K uint16 (MFMA B-operand order). */
int suo_pack_gemm_weight_bf16x3(const float* w, int N, int K, uint16_t* out);
int suo_conv1x1_bf16x3(const float* a_dev, int lda, int K, const float* pro_scale_dev, const float* pro_shift_dev, const uint16_t* wp3_dev,
                       const float* bias_dev, float* out_dev, int ldo, int M, int N, int relu, void* stream);
/* The general form: N a multiple of 128 (or 64), an optional second K segment (a2, K2: the skip conv of a Residual block; then no prologue), an optional
 * residual operand r_dev [M, ldr] added after the bias; K1, K2 multiples of 64; wp3 = suo_pack_gemm_weight_bf16x3 of the row-wise concatenation
 * [W1 | W2] (N rows, K1 + K2 columns).  What suo_net_forward launches for its N = 256 1x1 convolutions at 64x64 (lin, re-injection, conv3 + conv4). */
int suo_conv1x1_bf16x3_ex(const float* a1_dev, int lda1, int K1, const float* pro_scale_dev, const float* pro_shift_dev, const float* a2_dev,
                          int lda2, int K2, const uint16_t* wp3_dev, const float* bias_dev, const float* r_dev, int ldr, float* out_dev, int ldo,
                          int M, int N, int relu, void* stream);
/* ... with the 2x2 max-pool of the result written as well (suo_conv1x1_pool's contract: the M pixels are images of H x W, W a multiple of 64, H even;
 * pool_out_dev is [M/4, ldo]; out_dev may be NULL when only the pooled tensor is wanted). */
int suo_conv1x1_bf16x3_pool(const float* a1_dev, int lda1, int K1, const float* pro_scale_dev, const float* pro_shift_dev, const float* a2_dev,
                            int lda2, int K2, const uint16_t* wp3_dev, const float* bias_dev, const float* r_dev, int ldr, float* out_dev, int ldo,
                            int M, int N, int relu, int H, int W, float* pool_out_dev, void* stream);
/* The same kernel on TWO fp16 terms per operand, three MFMAs per product block (csrc/f16x2.h; what suo_net_forward launches by default).
 * w16 = suo_pack_gemm_weight_f16x2(W[N][K]) -> 2*N*K uint16 (row n times 2^t_n, max |row| in [2^12, 2^13)) and oscale[N] = 2^-(t_n + 4), the factor the
 * kernel's epilogue applies (activations enter times 2^4).  range_flag_dev: a device-visible word the kernel sets to 1 when a scaled activation reaches
 * 65504 (the launch's results are then invalid: re-issue on the bf16x3 entry); never cleared by the library. */
int suo_pack_gemm_weight_f16x2(const float* w, int N, int K, uint16_t* out, float* oscale_out);
int suo_conv1x1_f16x2_ex(const float* a1_dev, int lda1, int K1, const float* pro_scale_dev, const float* pro_shift_dev, const float* a2_dev, int lda2, int K2,
                         const uint16_t* w16_dev, const float* oscale_dev, const float* bias_dev, const float* r_dev, int ldr, float* out_dev, int ldo, int M, int N,
                         int relu, unsigned* range_flag_dev, void* stream);
int suo_conv1x1_f16x2_pool(const float* a1_dev, int lda1, int K1, const float* pro_scale_dev, const float* pro_shift_dev, const float* a2_dev, int lda2, int K2,
                           const uint16_t* w16_dev, const float* oscale_dev, const float* bias_dev, const float* r_dev, int ldr, float* out_dev, int ldo, int M, int N,
                           int relu, int H, int W, float* pool_out_dev, unsigned* range_flag_dev, void* stream);
/* KxK convolution, NHWC: KS=3 (stride 1, pad 1) or KS=7 (stride 2, pad 3) */
int suo_conv_kxk(int KS, const float* in_dev, int L, int H, int W, int C, const float* wp_dev, const float* bias_dev,
                 float* out_dev, int N, int relu, void* stream);
/* 3x3 convolution (stride 1, pad 1, N = 128 or 64 output channels, C a multiple of 16) in Winograd F(2x2,3x3) form: weight W[N][C][3][3] ->
 * out[16 * Np * Cp] floats (U = G g G^T per channel pair, computed in fp64, MFMA B-operand order); same tensors as suo_conv_kxk. */
int suo_pack_wino_weight(const float* w, int N, int C, int Np, int Cp, float* out);
int suo_conv3x3_wino(const float* in_dev, int L, int H, int W, int C, const float* wp_dev, const float* bias_dev, float* out_dev, int N,
                     int relu, void* stream);
/* The tail of a Residual block in ONE launch (layers/Residual.py:27-35): out = W3 relu(conv3x3(in) + bias2) + bias3 + skip with
 * in [L,H,W,128], out / skip [L,H,W,256] NHWC; the 128-channel tensor between the two convolutions stays in the CU.  Large
 * launches only (>= 1024 tiles of 128 pixels, the shapes the network uses it for); bit-identical to suo_conv_kxk + suo_conv1x1. */
int suo_conv3x3_conv1x1_skip(const float* in_dev, int L, int H, int W, const float* wp2_dev, const float* bias2_dev, const float* wp3_dev,
                             const float* bias3_dev, const float* skip_dev, float* out_dev, void* stream);
/* csrc/conv_wino_x3.hip (what suo_net_forward launches for the Residual blocks' 3x3 + tail unless SUO_WINO_BF16X3=0): the Winograd 3x3
 * convolution (128 -> 128 channels) with its element-wise products on the bf16 matrix pipe at fp32 accuracy (3-way split of both operands,
 * 6 of 9 cross terms, fp32 accumulate).
 * wq3 = suo_pack_wino_weight_bf16x3(W[128][128][3][3]) -> 3 * 16 * N * C uint16; same tensors as suo_conv3x3_wino / .._conv1x1_skip_up. */
int suo_pack_wino_weight_bf16x3(const float* w, int N, int C, uint16_t* out);
int suo_conv3x3_wino_x3(const float* in_dev, int L, int H, int W, const uint16_t* wq3_dev, const float* bias_dev, float* out_dev, int relu,
                        void* stream);
/* the same with channels = 128 or 64 (64 -> 64: the first two Residual blocks; wq3 = suo_pack_wino_weight_bf16x3(w, 64, 64, ...)) */
int suo_conv3x3_wino_x3_n(const float* in_dev, int L, int H, int W, int channels, const uint16_t* wq3_dev, const float* bias_dev, float* out_dev,
                          int relu, void* stream);
/* wp3_dev: conv3 weight packed by suo_pack_gemm_weight (tail_bf16x3 = 0: conv3 on the fp32 pipe) or by suo_pack_tail_weight_bf16x3
 * (tail_bf16x3 = 1: W3[256][128] -> 3 * 256 * 128 uint16, conv3 on the bf16 pipe as well). */
int suo_pack_tail_weight_bf16x3(const float* w3, int N2, int K, uint16_t* out);
int suo_conv3x3_wino_x3_conv1x1_skip_up(const float* in_dev, int L, int H, int W, const uint16_t* wq3_dev, const float* bias2_dev,
                                        const void* wp3_dev, int tail_bf16x3, const float* bias3_dev, const float* skip_dev,
                                        const float* up_dev, float* out_dev, void* stream);
/* csrc/conv_wino_x3.hip on two fp16 terms per operand (csrc/f16x2.h; the network's default for the Residual blocks' 3x3 + tail): packers return the planes
 * (2 * 16 * N * C / 2 * N2 * K uint16) and the per-output-channel factors; range_flag_dev as suo_conv1x1_f16x2_ex.
 * Launches of at most 256 tiles of 8 x 16 pixels (one workgroup per CU: a one-frame call, the passes of a SLAM view) run the 128-channel kernels with EIGHT waves
 * per tile (two per 32-channel slice, half the Winograd components each, no per-chunk fold; conv3 one 32-channel tile per wave): the same products, the last
 * additions of the output transform paired differently -- results within fp32 rounding of the four-wave form's, which SUO_WINO_W8=0 keeps everywhere. */
int suo_pack_wino_weight_f16x2(const float* w, int N, int C, uint16_t* out, float* oscale_out);
int suo_conv3x3_wino_f16x2_n(const float* in_dev, int L, int H, int W, int channels, const uint16_t* wq16_dev, const float* oscale_dev, const float* bias_dev,
                             float* out_dev, int relu, unsigned* range_flag_dev, void* stream);
int suo_pack_tail_weight_f16x2(const float* w3, int N2, int K, uint16_t* out, float* oscale_out);
int suo_conv3x3_wino_f16x2_conv1x1_skip_up(const float* in_dev, int L, int H, int W, const uint16_t* wq16_dev, const float* oscale2_dev, const float* bias2_dev,
                                           const uint16_t* w3p16_dev, const float* oscale3_dev, const float* bias3_dev, const float* skip_dev, const float* up_dev,
                                           float* out_dev, unsigned* range_flag_dev, void* stream);
/* ... and with the NEXT Residual block's conv1 in the same launch (layers/Residual.py:22-24 of the block that consumes out_dev): next_out_dev [L,H,W,128] =
 * relu(W1' relu(out * next_scale + next_shift) + next_b1) with W1' [128][256] (bn1 folded) as suo_pack_gemm_weight_f16x2 planes + factors.  out_dev is written as
 * before; the 256-channel tensor is not re-read by a separate 1x1 launch.  Bit-identical to suo_conv3x3_wino_f16x2_conv1x1_skip_up followed by
 * suo_conv1x1_f16x2_ex (same products, same order).  What suo_net_forward launches wherever a 256 -> 256 block on a launch of more than 256 tiles feeds another
 * (always the four-wave kernel: the eight-wave form of small launches does not carry the next block's conv1). */
int suo_conv3x3_wino_f16x2_conv1x1_skip_up_next(const float* in_dev, int L, int H, int W, const uint16_t* wq16_dev, const float* oscale2_dev, const float* bias2_dev,
                                                const uint16_t* w3p16_dev, const float* oscale3_dev, const float* bias3_dev, const float* skip_dev, const float* up_dev,
                                                float* out_dev, const float* next_scale_dev, const float* next_shift_dev, const uint16_t* next_w1h_dev,
                                                const float* next_osc1_dev, const float* next_b1_dev, float* next_out_dev, unsigned* range_flag_dev, void* stream);
/* The same with the 3x3 convolution in Winograd form (wq2 from suo_pack_wino_weight): what the network launches for its 256 -> 256 blocks */
int suo_conv3x3_wino_conv1x1_skip(const float* in_dev, int L, int H, int W, const float* wq2_dev, const float* bias2_dev, const float* wp3_dev,
                                  const float* bias3_dev, const float* skip_dev, float* out_dev, void* stream);
/* ... and with the Hourglass's "up1 + up2(low3)" (hg.py:56-58) folded in: out += nearest-neighbour 2x up-sampling of up_dev [L,H/2,W/2,256] */
int suo_conv3x3_wino_conv1x1_skip_up(const float* in_dev, int L, int H, int W, const float* wq2_dev, const float* bias2_dev, const float* wp3_dev,
                                     const float* bias3_dev, const float* skip_dev, const float* up_dev, float* out_dev, void* stream);
/* csrc/res_small.hip (what suo_net_forward launches for the Hourglass blocks at 32x32 and below when a call holds few crops -- the reference's
 * call shape, one frame per call, lib/object_slam.py:1099): a WHOLE 256 -> 256 Residual block (layers/Residual.py:20-35) in one launch,
 *   out = W3 relu(conv3x3(relu(W1 relu(x * pro_scale + pro_shift) + b1)) + b2) + b3 + x [+ 2x up-sampling of up_dev]
 * x_dev [L,H,W,256] NHWC -- or, pool_in = 1, [L,2H,2W,256] whose 2x2 max-pool is the block's input (hg.py:41).  Weights with their
 * BatchNorms folded by the caller: w1 [128][256], w2 [128][128][3][3] (times scale2[n] if given), w3 [256][128], packed by
 * suo_pack_res_block into w1p [128*256], w2p [128*128*9], w3p [256*128] floats.  Bit-identical to suo_conv1x1 (prologue, ReLU) ->
 * suo_conv_kxk(3) (ReLU) -> suo_conv1x1 (+ skip) -> suo_upsample2_add on the same tensors. */
int suo_pack_res_block(const float* w1, const float* w2, const float* scale2, const float* w3, float* w1p, float* w2p, float* w3p);
int suo_res_block(const float* x_dev, int L, int H, int W, int pool_in, const float* pro_scale_dev, const float* pro_shift_dev, const float* w1p_dev,
                  const float* b1_dev, const float* w2p_dev, const float* b2_dev, const float* w3p_dev, const float* b3_dev, const float* up_dev,
                  float* out_dev, void* stream);
/* csrc/res_small_x3.hip: the same block with every product on the bf16 matrix pipe at fp32 accuracy (3-way operand split, csrc/bf16x3.h), 4 x 8 pixel
 * tiles -- the network's default for the 32x32 and 16x16 levels of a one-frame call.  Weights as uint16 planes: w1x [3*128*256], w2x [3*128*128*9],
 * w3x [3*256*128] from suo_pack_res_block_bf16x3 (same inputs as suo_pack_res_block). */
int suo_pack_res_block_bf16x3(const float* w1, const float* w2, const float* scale2, const float* w3, uint16_t* w1x, uint16_t* w2x, uint16_t* w3x);
int suo_res_block_bf16x3(const float* x_dev, int L, int H, int W, int pool_in, const float* pro_scale_dev, const float* pro_shift_dev,
                         const uint16_t* w1x_dev, const float* b1_dev, const uint16_t* w2x_dev, const float* b2_dev, const uint16_t* w3x_dev,
                         const float* b3_dev, const float* up_dev, float* out_dev, void* stream);
/* ... and on two fp16 terms per operand (csrc/f16x2.h; the default of suo_net_forward for these levels): planes w1h [2*128*256], w2h [2*128*128*9], w3h [2*256*128]
 * and the per-channel factors osc1 [128], osc2 [128], osc3 [256] from suo_pack_res_block_f16x2; range_flag_dev as suo_conv1x1_f16x2_ex (here it also covers the
 * two activations the caller never sees, relu(conv1) and relu(conv2)). */
int suo_pack_res_block_f16x2(const float* w1, const float* w2, const float* scale2, const float* w3, uint16_t* w1h, uint16_t* w2h, uint16_t* w3h, float* osc1, float* osc2,
                             float* osc3);
int suo_res_block_f16x2(const float* x_dev, int L, int H, int W, int pool_in, const float* pro_scale_dev, const float* pro_shift_dev, const uint16_t* w1h_dev,
                        const float* osc1_dev, const float* b1_dev, const uint16_t* w2h_dev, const float* osc2_dev, const float* b2_dev, const uint16_t* w3h_dev,
                        const float* osc3_dev, const float* b3_dev, const float* up_dev, float* out_dev, unsigned* range_flag_dev, void* stream);
/* csrc/gemm_bf16x3.hip (gemm_chain_head_kernel): TWO 1x1 convolutions in one launch -- the last stack's  logits = tmpOut(relu(bn(lin(x))))  (hg.py:106-111) -- with the
 * 256-channel tensor between them kept in LDS instead of written and read back (what suo_net_forward launches for it at >= 4096 pixels on the fp16 pipe (csrc/net.hip: x3_min_rows); SUO_CHAIN_HEAD=0: two launches).
 * a_dev [M, lda >= 256] rows; w1h / osc1 = suo_pack_gemm_weight_f16x2 of W1 [256][256] (BatchNorm folded), bias1 [256]; w2h / osc2 of W2 [64][256] (rows >= n_valid zero),
 * bias2 [64]; out_nchw_dev [M / hw, n_valid, hw].  M a multiple of 64, hw a multiple of 64 dividing M.  Bit-identical to suo_conv1x1_f16x2_ex twice. */
int suo_conv1x1_chain_head_f16x2(const float* a_dev, int lda, int M, const uint16_t* w1h_dev, const float* osc1_dev, const float* bias1_dev, const uint16_t* w2h_dev,
                                 const float* osc2_dev, const float* bias2_dev, float* out_nchw_dev, int n_valid, int hw, unsigned* range_flag_dev, void* stream);
/* csrc/stem_x3.hip (what suo_net_forward launches for the prior-less pass unless SUO_STEM_X3=0): RoIAlign of the frame (pkpnet.py:93) + the stem
 * conv1_ 7x7 / stride 2 over the 3 image channels + bn1 + ReLU (hg.py:67-69,96-98) in one launch, products on the bf16 matrix pipe (3-way split);
 * the staged [L,256,256,*] crop tensor is never written.  wx = suo_pack_stem_weight_bf16x3(W[64][Cw][7][7], Cw, bn scale[64] or NULL) ->
 * 14 * 2 * 3 * 64 * 8 uint16; bias [64] (folded); frame / boxes / box_img as suo_roi_align_concat; out_dev [L,128,128,64] NHWC. */
int suo_pack_stem_weight_bf16x3(const float* w, int Cw, const float* scale, uint16_t* out);
int suo_stem_x3(const void* img_dev, int fmt, int H, int W, const float* boxes_dev, const int* box_img_dev, int L, const uint16_t* wx_dev,
                const float* bias_dev, float* out_dev, void* stream);
/* ... on two fp16 terms per operand (csrc/f16x2.h; the default of suo_net_forward): wh = suo_pack_stem_weight_f16x2 -> 14 * 2 * 2 * 64 * 8 uint16 and oscale [64];
 * range_flag_dev as suo_conv1x1_f16x2_ex (a uint8 frame cannot raise it; a float frame holding values beyond 4094 does). */
int suo_pack_stem_weight_f16x2(const float* w, int Cw, const float* scale, uint16_t* out, float* oscale_out);
int suo_stem_f16x2(const void* img_dev, int fmt, int H, int W, const float* boxes_dev, const int* box_img_dev, int L, const uint16_t* wh_dev, const float* oscale_dev,
                   const float* bias_dev, float* out_dev, unsigned* range_flag_dev, void* stream);
/* ... with the first Residual block's conv1 computed on the tile as well (what suo_net_forward launches; SUO_STEM_NEXT=0: conv1 as its own launch):
 * n_out [L,128,128,64] = relu(W1 relu(n_scale * out + n_shift) * n_osc1 + n_b1), n_w1h / n_osc1 = suo_pack_gemm_weight_f16x2 of W1 [64][64] (BatchNorm folded).
 * Bit-identical to suo_stem_f16x2 followed by suo_conv1x1_f16x2_ex on its output. */
int suo_stem_f16x2_next(const void* img_dev, int fmt, int H, int W, const float* boxes_dev, const int* box_img_dev, int L, const uint16_t* wh_dev, const float* oscale_dev,
                        const float* bias_dev, float* out_dev, const float* n_scale_dev, const float* n_shift_dev, const uint16_t* n_w1h_dev, const float* n_osc1_dev,
                        const float* n_b1_dev, float* n_out_dev, unsigned* range_flag_dev, void* stream);
/* Tests only, not thread-safe.  Device pointers to 2^s (one float each; csrc/f16x2.h: a site's activation factor) that the per-stage f16x2 entries above put into
 * their kernel arguments from now on:
 *   in    - the entry's input site (suo_conv1x1_f16x2_ex / _pool, suo_conv3x3_wino_f16x2_n, conv2 of the fused tails, conv1 of suo_res_block_f16x2, lin of the chain head)
 *   inner - the second site: the tail's conv3, the block's conv2, the chain head's tmpOut
 *   third - the one-launch block's conv3
 *   next  - the NEXT conv1 of the tail and of the stem (the stem's own site keeps 2^4: its input is the frame)
 * NULL = the default 2^4; all four NULL restores the behaviour without the hook bit for bit.  The caller passes per-channel factors that belong to the shift
 * (ldexp(oscale, 4 - s) of what the packers return) and keeps the pointers alive while they are set.  suo_net_* never reads them. */
int suo_debug_f16x2_stage_sites(const float* in, const float* inner, const float* third, const float* next);
int suo_maxpool2(const float* in_dev, float* out_dev, int L, int H, int W, int C, void* stream);
int suo_upsample2_add(const float* up1_dev, const float* low_dev, float* out_dev, int L, int H, int W, int C, void* stream);

/* ---- PnP: replaces lambdatwist.pnp (thirdparty/lambdatwist/pnp_python_binding.cpp:32-62) ---------- */
/* One call per object in the reference (lib/object_slam.py:1144); here all objects of a frame go in one
 * launch (one wavefront each).  Host buffers: n_pts[n_obj]; xs [sum n_pts][3] model points; ys
 * [sum n_pts][2] NORMALISED image points (object_slam.py:34-36); threshold as PnpParams (1e-3).
 * T_out [n_obj][16] row-major 4x4.  status[o] = 1 <=> identity pose = total failure, the reference's
 * error convention (pnp_ransac.cpp:231, object_slam.py:38).  Objects with n_pts < 4 return identity.
 * seed keys the counter-based sampler (object o uses seed + o * 0x9E3779B97F4A7C15).  Never throws. */
int suo_pnp_batch(int n_obj, const int* n_pts, const double* xs, const double* ys, double threshold, uint64_t seed,
                  int do_refine, double* T_out, int* status, int* best_inliers, int* iterations);
/* Index-work parity with the reference's sampler (legacy entry, not the batched fast path): the same RANSAC with hypothesis i of object o sampling the four
 * points draws[(o * n_draws + i) * 4 .. + 3] (ascending indices into the object's points) instead of the counter-based generator.  Fed with the sequence the
 * reference's process-global std::default_random_engine (seed 0) gives through get4RandomInRange0 (thirdparty/lambdatwist/pnp_ransac.cpp:161-183,
 * utils/random.h:65-116; restated host-side in suo_slam_amd/lambdatwist.py: ReferenceSampler) the chosen sample and the consensus set are the reference's.
 * n_draws >= 1000 (the iteration cap, parameters.h:76-102); winner[o] = index of the hypothesis that became the result, -1 if none; host buffers. */
int suo_pnp_replay(int n_obj, const int* n_pts, const double* xs, const double* ys, double threshold, const int* draws, int n_draws, int do_refine,
                   double* T_out, int* status, int* best_inliers, int* iterations, int* winner);
/* exact legacy signature: pnp(xs[N,3], ys[N,2], threshold) -> 4x4 */
int suo_pnp(const double* xs, const double* ys, int n, double threshold, double* T_out);

/* ---- device-resident frame geometry: network outputs -> poses in one stream-ordered chain ----------------------
 * What the reference does on the host between the network and the poses of a single-view frame -- the three .cpu() synchronisations
 * and mask logic (lib/object_slam.py:1100-1115), `exp_uv[k][kp_mask]` compaction (:1118-1135), the K^-T normalisation of pnp() (:34-36),
 * one lambdatwist.pnp per object (:1144), acceptance (:1147-1148), then optimize(): one g2o edge per keypoint with inv(cov) as
 * information (:795-837) and the robust LM rounds (:842-896) with the camera fixed at identity (:383-385, :774) -- as four kernels on the
 * caller's stream behind suo_net_forward* + suo_keypoint_masks, and ONE device-to-host copy of everything the host keeps.
 *   suo_frame_geom_launch: asynchronous.  n_frames frames, frame f = crops [frame_first[f], frame_first[f+1]) of the device arrays
 *     uv_dev [L,41,2], cov_dev [L,41,2,2], mask_dev [L,41] (the network's outputs and suo_keypoint_masks' result, same stream),
 *     model_kps_dev float32 [L,41,3].  Host arrays (copied before returning): kinv [L][6] = KinvT[0][0],[1][0],[2][0],[0][1],[1][1],[2][1]
 *     of inv(K_bbox).T (:34), camk [L][4] = fx, fy, cx, cy of K_bbox (:799), min_depth [L] = 0.5 * diameter (:1147).
 *     PnP sampler keys as if suo_pnp_batch were called once per frame with that frame's solvable crops (>= 4 keypoints) only and the
 *     caller advanced `seed` by their number from frame to frame (what ObjectSLAM does between process_view calls).
 *     do_lm = 0 stops after PnP + acceptance (SLAM tracking continues on the host: camera hypotheses :975-1072).
 *     At most 16 crops per frame when do_lm (one wave per object, csrc/lm_frame.hip).
 *     Singular covariances (DEVIATION: the reference's np.linalg.inv raises LinAlgError on the exactly singular ones, :827, and hands g2o whatever it returns for
 *     the others): with use_cov, a keypoint whose float32 covariance [[a, b], [c, d]] gives a det = a d - b c in fp64 (products exact, one rounding) that is not
 *     finite or is <= 0 is not a measurement.  The chain treats it as masked out: it is not a PnP point, not a graph edge, does not count in n_kp and reads
 *     back as mask = 0, whatever mask_dev said (suo_keypoint_masks lets a zero variance through: sqrt(0) < 2 kp_var_thresh).  An invertible covariance is
 *     untouched, bit for bit.  With use_cov = 0 the covariance is not read and the keypoint stays.  The host-array route (suo_pnp_batch + suo_optimize with
 *     information matrices the caller inverted, ObjectSLAM(device_chain=False)) keeps np.linalg.inv and its exception.
 *   suo_frame_geom_fetch: waits for that launch and points `out` into the context's pinned read-back block (valid until the next launch):
 *     per crop T_pnp [16] (row-major 4x4; pnp_status 1 = identity = failure), accepted, T_opt [12] (refined T_OtoC, = PnP pose when not
 *     refined), n_kp, and per keypoint SLOT (crop * 41 + position among the crop's valid keypoints, i.e. the order of the reference's
 *     boolean indexing) inlier / chi2; uv / cov / mask as the network and suo_keypoint_masks wrote them; lm_stats [n_frames][4]. */
typedef struct suo_frame_geom suo_frame_geom;
typedef struct suo_frame_geom_params {
    double pnp_threshold;          /* 1e-3 (parameters.h:35) */
    uint64_t seed;
    int use_cov;                   /* 0: information = identity (no_network_cov, :825) */
    int do_lm;
    int its[4]; int n_rounds;      /* {10,10,40,40}, 4 (:843-846) */
    double chi2_thr;               /* 5.991 */
    double huber_delta;            /* sqrt(5.991) */
    uint64_t* seed_dev;            /* NULL, or a device-resident running key: the launch samples with seed + *seed_dev (read when its PnP kernel runs) and
                                    * adds its number of solvable problems (crops with >= 4 keypoints) to *seed_dev when done -- what a host caller adds to
                                    * `seed` between launches, without waiting for the previous launch's read-back (a second batch in flight) */
} suo_frame_geom_params;
typedef struct suo_frame_geom_result {
    int n_frames, n_crops;
    const double* T_pnp; const double* T_opt; const double* chi2;
    const int* pnp_status; const int* pnp_best_inliers; const int* pnp_iterations; const int* n_kp; const int* lm_stats;
    const uint8_t* accepted; const uint8_t* inlier;
    const float* uv; const float* cov; const uint8_t* mask;
    const double* obj_cov;         /* [n_crops][36] after suo_frame_geom_covariances, NULL without it */
} suo_frame_geom_result;
int suo_frame_geom_create(int max_crops, int max_frames, suo_frame_geom** out);
void suo_frame_geom_destroy(suo_frame_geom* g);
int suo_frame_geom_launch(suo_frame_geom* g, int n_frames, const int* frame_first, const float* uv_dev, const float* cov_dev,
                          const uint8_t* mask_dev, const float* model_kps_dev, const double* kinv, const double* camk, const double* min_depth,
                          const suo_frame_geom_params* params, void* stream);
int suo_frame_geom_fetch(suo_frame_geom* g, suo_frame_geom_result* out);
int suo_frame_geom_ready(suo_frame_geom* g);      /* 1 when the last launch has completed (or nothing is in flight), 0 otherwise; never blocks */
/* The result block's DEVICE pointers (same fields): valid, stream-ordered, for work enqueued on the launch's stream behind it, until the context's next launch. */
int suo_frame_geom_device_result(suo_frame_geom* g, suo_frame_geom_result* out);
/* Optional, asynchronous, after suo_frame_geom_launch and on the SAME stream: the 6x6 covariance of every crop's refined pose (definition: suo_pose_covariances
 * below; a single-view frame has no free camera, so every accepted crop is a block of its own) from the device-resident graph of the last launch, at the poses
 * and inlier flags its LM left (do_lm = 0: at the PnP poses, every keypoint counted).  suo_frame_geom_fetch then waits for it too and obj_cov of both result
 * calls points at [n_crops][36] row-major doubles: zeros for a crop that was not accepted, NaNs for an accepted crop without a counted keypoint or with a
 * singular block.  Without this call obj_cov is NULL and nothing else differs. */
int suo_frame_geom_covariances(suo_frame_geom* g, void* stream);

/* ---- SLAM tracking between the two network passes of a view (round 6): camera-hypothesis vote + prior projection on the device -------------
 * Replaces, on the caller's stream and without a host round trip, ObjectSLAM.__estimate_camera_pose (lib/object_slam.py:975-1072) on the detections of the view's
 * FIRST pass and the projection of the prior keypoints of the SECOND pass's objects (:486-514).  Inputs on the device: pass A's chain results
 * (suo_frame_geom_device_result: T_pnp [n_a][16], accepted [n_a], n_kp [n_a]), pass A's network outputs uv / cov, its masks and model keypoints ([n_a,41,...]), pass B's
 * model keypoints [n_b,41,3] float32 and class masks [n_b,41]; block_dev = SUO_SLAM_VOTE_BLOCK doubles staged by the caller (e.g. with its other small arrays):
 *   a_in_map [16] | a_T_OtoG [16][12] | a_K_bbox [16][9] (the float32 container widened, :1082) | b_in_map [16] | b_T_OtoG [16][12] | b_K_bbox [16][9] (fix_K_for_bbox_ndc, double)
 * (rows of objects that are not in the map: in_map 0, the rest ignored).  has_cov / kp_std2 / chi2_max as suo_slam_score; min_inliers = 4 (:975).
 * Outputs on the device: prior_uv_dev [n_b][41][2] float32 + prior_mask_dev [n_b][41] -- what suo_net_forward_prior_kp takes (rows of objects without a prior: zeros) --
 * and out_dev [SUO_SLAM_VOTE_OUT] doubles: T_GtoC [3][4] | best crop (-1: no hypothesis reached min_inliers -- the caller falls back to
 * __backup_estimate_camera_pose and issues pass B again) | number of hypotheses | best count | counts [16] (-1: not a hypothesis) | NaN flag.
 * n_kp_dev is accepted for the chain's result block as it stands and NOT READ (it may be null): a crop's keypoints are those of its mask, in mask order.  The variances
 * are clamped as np.maximum clamps them -- a NaN variance stays a NaN and sets the flag, as any NaN chi-square of a keypoint in front of the camera does.
 * What "equal to the host route" means is tested directly (tests/test_gpu_slam_vote.py): T_GtoC and the priors are bit-identical to the documented arithmetic
 * (csrc/slam_vote.hip's header; restated exactly in tests/slam_vote_ref.py), the counts are exact against the reference's rule.
 * SUO_ERR_ARG (nothing launched): n_a or n_b outside 1..16, or a null pointer other than n_kp_dev / stream. */
#define SUO_SLAM_VOTE_BLOCK 704
#define SUO_SLAM_VOTE_OUT 32
int suo_slam_vote(int n_a, const double* T_pnp_dev, const uint8_t* accepted_dev, const int* n_kp_dev, const float* uv_dev, const float* cov_dev,
                  const uint8_t* mask_dev, const float* model_kps_a_dev, const double* block_dev, int n_b, const float* model_kps_b_dev,
                  const uint8_t* model_mask_b_dev, int has_cov, double kp_std2, double chi2_max, int min_inliers, float* prior_uv_dev,
                  uint8_t* prior_mask_dev, double* out_dev, void* stream);

/* ---- pose refinement / bundle adjustment: replaces the g2o calls of ObjectSLAM.optimize -------------
 * (lib/object_slam.py:703-903; g2o surface listed in SURVEY.md 8b).  A problem is the flat SoA of the graph
 * the reference builds edge by edge (:746-839): vertices = cameras (T_GtoC) and objects (T_OtoG) as
 * row-major 3x4; one edge per keypoint measurement with cam_k = [fx,fy,cx,cy] of K_bbox, model point,
 * measured uv (NDC) and information (xx,xy,yy).  obj_fixed all 1 reproduces curr_only mode
 * (EdgeSE3ProjectFromFixedObject); cam_fixed[0]=1 the global / single-view gauge (:774).
 * Runs the robust rounds of :842-896 (its[], chi2 gate, Huber drop at round max(1,n_rounds/2)) on-device. */
typedef struct suo_ba_problem {
    int n_cam, n_obj, n_edge;
    double* cam_T;                 /* [n_cam][12] in/out */
    const uint8_t* cam_fixed;      /* [n_cam] */
    double* obj_T;                 /* [n_obj][12] in/out */
    const uint8_t* obj_fixed;      /* [n_obj] */
    const int32_t* edge_cam;       /* [n_edge] */
    const int32_t* edge_obj;       /* [n_edge] */
    const double* edge_camk;       /* [n_edge][4] */
    const double* edge_p;          /* [n_edge][3] */
    const double* edge_uv;         /* [n_edge][2] */
    const double* edge_info;       /* [n_edge][3] = (xx, xy, yy) */
    uint8_t* edge_inlier;          /* [n_edge] in/out (detections[...]["inliers"]) */
    double* edge_chi2;             /* [n_edge] out, may be NULL */
    int its[8]; int n_rounds;      /* e.g. {10,10,40,40}, 4 */
    int init_with_outliers;        /* opt_init_with_outliers and curr_only (:848-852) */
    double chi2_thr;               /* 5.991 */
    double huber_delta;            /* sqrt(5.991) */
    int stats[4];                  /* out: rounds, LM iterations, LM trials, final num_good */
} suo_ba_problem;
int suo_optimize(suo_ba_problem* problem);
/* many independent problems (frames) in one launch, one workgroup each.
 * Which kernels run (all of them g2o's Levenberg-Marquardt on the same graph, optimization_algorithm_levenberg.cpp:58-150; they differ in summation order only):
 *   frame-sized graphs (the per-view refinements)                       one 256-thread workgroup per problem (csrc/lm.hip)
 *   ONE graph of >= 512 edges with free cameras and free objects        the phase kernels of the multi-GPU adjustment below on one rank under the device-resident
 *   (ObjectSLAM.optimize's global adjustment, lib/object_slam.py:746)   schedule, driven from C: ~12 launches per LM trial, the host reads 16 doubles once per <= 12 trials
 *                                                                       (round 6; 60 cameras x 8 objects: 6.8 ms)
 *   more than 16 free objects next to free cameras                      the same phases under the host-driven schedule (the reduced system then lives in HBM) */
int suo_optimize_batch(suo_ba_problem* problems, int n_problems);
/* Test entry: the kernel suo_optimize_batch runs each problem of this batch on -- the plan the dispatcher itself executes (csrc/ba_api.hip: plan_ba_batch; same
 * thresholds, same SUO_LM_CAM2), reported instead of run; launches nothing and needs no device.  A batch runs on ONE kernel, except that a batch holding a PHASEWISE graph runs its other problems one by
 * one, each on the route it takes alone.  route_out[i] is a SUO_LM_ROUTE_* code; lds_need_out (may be NULL) [i] is, on the LM / LM_BIG routes, the dynamic LDS
 * in bytes that a fully resident problem asks for BEFORE the 150 KiB cap (the kernel relocates arrays into LDS while they fit), -1 on the others. */
#define SUO_LM_ROUTE_LM 0          /* lm_kernel, 256 threads (csrc/lm.hip): what no route below takes, < 512 edges */
#define SUO_LM_ROUTE_LM_BIG 1      /* lm_kernel, 1024 threads (csrc/lm_big.hip): the same with >= 512 edges in some problem */
#define SUO_LM_ROUTE_FRAME2 2      /* lm_frame2_kernel: one fixed camera, <= 16 objects, one wave per frame */
#define SUO_LM_ROUTE_FRAME8 3      /* lm_frame_kernel<8>: no free camera, one wave per object, <= 8 objects in every problem */
#define SUO_LM_ROUTE_FRAME16 4     /* lm_frame_kernel<16>: the same with 9-16 objects in some problem */
#define SUO_LM_ROUTE_CAM2 5        /* lm_cam2_kernel: one free camera alone in its graph, every object fixed, <= 1024 edges */
#define SUO_LM_ROUTE_CAM 6         /* lm_cam_kernel: one free camera, every object fixed, otherwise */
#define SUO_LM_ROUTE_PHASES 7      /* csrc/lm_dist.hip phases, device-resident schedule: ONE graph of >= 512 edges, free cameras and free objects */
#define SUO_LM_ROUTE_PHASEWISE 8   /* the same phases under the host schedule: > 16 free objects next to free cameras */
int suo_debug_lm_routes(const suo_ba_problem* problems, int n_problems, int* route_out, int* lds_need_out);

/* ---- 6x6 pose covariances of the refined cameras and objects ----------------------------------------------------------------------
 * The state is the one the suo_ba_problem holds, i.e. cam_T, obj_T and edge_inlier as suo_optimize leaves them.
 *   Hessian.     H is the sum of J^T Omega J over edges whose edge_inlier is 1 and whose camera and object are not both fixed.  There is no Huber weight and no
 *                lambda.  The columns of J are [omega, upsilon] of the left-multiplicative update exp(delta) * T, restricted to free vertices: the convention
 *                suo_debug_ba_jacobians documents and csrc/lm_device.h implements.
 *   Covariance.  Sigma = H^-1.  The result is the 6x6 diagonal block of Sigma for every camera and every object, as 36 row-major doubles per vertex:
 *                - fixed vertex: 36 zeros;
 *                - free vertex with no counted edge, or a system whose factorisation meets a non-positive pivot: 36 NaNs for every affected block, and `status`
 *                  counts them.  Vertices in other connected blocks are unaffected.  The call never faults and never loops on a bad pivot.
 *                  (Affected: without a free camera, or without a free object, every vertex is a block of its own; where free cameras meet free objects, a vertex
 *                  without a counted edge is left out of the system, and a bad pivot of what remains marks every free vertex of that problem.)
 *                - the chi2 scale is not applied: this is the covariance under the stated information matrices.  suo_residual_statistics below reports the scale
 *                  (summary[5] = s0^2); a caller who wants the scaled covariance multiplies.
 * Host buffers, blocking, staged through the arena of suo_optimize_batch; the problem is not modified (its, n_rounds, chi2_thr, huber_delta, stats are not read).
 * cam_cov [n_cam][36], obj_cov [n_obj][36] (either may be NULL), status [2] = number of NaN camera blocks, NaN object blocks (may be NULL); the batch form takes
 * one pointer per problem and status [n][2], and gives every problem the bits it gets alone.  Kernels (csrc/pose_cov.hip, fp64, fixed summation order):
 *   no free camera (single-view frames, any number of objects)    one wave per problem, 8 / 4 lanes per object, passes of 16 objects
 *   no free object (camera tracking, curr_only graphs)            the same over the cameras
 *   free cameras next to <= 16 free objects                       one workgroup per problem: Schur complement onto the objects, the LM kernels' block-6 Cholesky once,
 *                                                                  Sigma_OO = S^-1 in LDS, Sigma_cc = Hcc^-1 + Y Sigma_OO Y^T per camera
 *   free cameras next to more than 16 free objects                SUO_ERR_ARG (the reduced system and its inverse no longer fit the LDS); nothing is launched */
int suo_pose_covariances(const suo_ba_problem* problem, double* cam_cov /*[n_cam][36]*/, double* obj_cov /*[n_obj][36]*/, int* status /*[2]: NaN cam blocks, NaN obj blocks*/);
int suo_pose_covariances_batch(const suo_ba_problem* problems, int n, double* const* cam_cov, double* const* obj_cov, int* status /*[n][2]*/);

/* ---- cross blocks and relative-pose covariances of vertex pairs ---------------------------------------------------------------------
 * The marginal blocks above are expressed relative to whichever camera is fixed (the gauge).  The pose of an object in a camera's frame, and of one object
 * relative to another, do not depend on that choice, and neither do their covariances; they need the off-diagonal blocks of Sigma.
 *   Vertices.    One index codes a vertex: camera c is c, object o is n_cam + o.
 *   Perturbation. The library's: left update exp(delta) * T, delta = [omega, upsilon].  Ad(T) = [[R, 0], [[t]x R, R]].
 *   Pairs.       (camera c, object o), in either order:  T_OtoC = T_c * T_o,      delta_rel = delta_c + Ad(T_c) delta_o,
 *                                                         rel = Sigma_cc + A Sigma_oo A^T + Sigma_co A^T + A Sigma_oc,   A = Ad(T_c)
 *                (object a, object b):                    T_AtoB = T_b^-1 * T_a,   delta_rel = B (delta_a - delta_b),
 *                                                         rel = B (Sigma_aa + Sigma_bb - Sigma_ab - Sigma_ba) B^T,       B = Ad(T_b^-1)
 *                (camera, camera): SUO_ERR_ARG, nothing is launched.
 *   cross [n_pair][36]  Sigma_ab: rows are vertex a, columns are vertex b, row-major.  (a, a) is the marginal block.
 *   rel   [n_pair][36]  as above, exactly symmetric.  Either may be NULL.
 *   - A fixed vertex contributes zeros: a pair with the gauge camera reduces to A Sigma_oo A^T, a pair with a fixed object to Sigma_cc, two fixed objects to 36 zeros.
 *   - Both blocks of a pair are 36 NaNs if a vertex of the pair is NaN in the marginal call; status[2] counts those pairs.
 *   - An index outside [0, n_cam + n_obj), a (camera, camera) pair or n_pair < 0: SUO_ERR_ARG.  Duplicate pairs are allowed.  n_pair == 0 is suo_pose_covariances.
 *   - cam_cov / obj_cov / status[0..1] are those of suo_pose_covariances, bit for bit; more than 16 free objects next to free cameras: SUO_ERR_ARG, as there.
 * Buffers, blocking and arena as suo_pose_covariances.  Kernels (csrc/pose_cov.hip, fp64, fixed summation order, two calls give the same bits, a problem's pairs
 * do not depend on the rest of the batch): without a free camera or without a free object every cross block between two vertices is zero; in the coupled form the
 * camera waves write Sigma_co = -(Y Sigma_OO)[:, o] -- dense over the objects, also where the camera does not see the object -- and Sigma_ab comes from Sigma_OO;
 * one small kernel behind them propagates.  The batch form takes one pointer (and one n_pair) per problem and status [n][3]. */
int suo_pose_covariances_pairs(const suo_ba_problem* problem, int n_pair, const int32_t* pair_a, const int32_t* pair_b, double* cam_cov /*[n_cam][36]*/,
                               double* obj_cov /*[n_obj][36]*/, double* cross /*[n_pair][36]*/, double* rel /*[n_pair][36]*/,
                               int* status /*[3]: NaN cam blocks, NaN obj blocks, NaN pairs*/);
int suo_pose_covariances_pairs_batch(const suo_ba_problem* problems, int n, const int* n_pair, const int32_t* const* pair_a, const int32_t* const* pair_b,
                                     double* const* cam_cov, double* const* obj_cov, double* const* cross, double* const* rel, int* status /*[n][3]*/);

/* ---- pose covariances of maps beyond 16 objects and between cameras ----------------------------------------------------------------
 * suo_pose_covariances_graph is suo_pose_covariances_pairs -- the same Hessian, perturbation, vertex coding, zeros for fixed vertices, NaN rules, status [3],
 * buffers and blocking -- with its two refusals lifted:
 *   Free objects.  Any number of free objects next to free cameras up to SUO_POSE_COV_GRAPH_MAX_OBJ = 64.  The cap is what the scratch costs: the reduced system
 *                and its inverse live in the arena, 2 * 8 * (6 * 64)^2 bytes = 2.4 MB per problem at the cap (device and pinned host mirror), and a lane of the
 *                column kernel holds 6 * cap / 64 = 6 elements of a row of the factor in registers.  More: SUO_ERR_ARG naming the count and the cap, nothing is launched.
 *   (camera a, camera b):  T_AtoB = T_b * T_a^-1,   delta_rel = delta_b - A delta_a,   A = Ad(T_b T_a^-1)
 *                          rel = Sigma_bb + A Sigma_aa A^T - A Sigma_ab - Sigma_ba A^T
 *                          cross = Sigma_ab: rows are vertex a, columns are vertex b.
 *   - A fixed camera contributes zeros: (gauge, c) gives Sigma_cc, (c, gauge) gives A Sigma_cc A^T, two fixed cameras 36 zeros.
 *   - (c, c): cross is the marginal block and rel is 36 zeros exactly.
 *   - Where free cameras meet free objects, Sigma_cc' (c != c') = Y_c Sigma_OO Y_c'^T: dense, also where the two cameras share no object.
 *     Without a free object the cross block of two cameras is zero and rel comes from the marginal blocks.
 *   - (a, b) is the transpose of (b, a) to the bit, as for the object pairs.
 *   - A pair touching a NaN vertex gives 36 NaNs in both blocks and is counted in status[2].
 *   Bits.        A problem that suo_pose_covariances_pairs answers and that has no (camera, camera) pair runs on the kernels of that entry: every output is
 *                bit-identical to it.  Every other problem with free cameras next to free objects runs on the device-memory form, whatever its object count.
 *                A problem's result does not depend on the rest of the batch, and two calls give the same bits.
 * Kernels (csrc/pose_cov_graph.hip, fp64, fixed summation order, vector stores only): S, S^-1 = Sigma_OO and every camera's Z = Y Sigma_OO in device memory; one
 * workgroup per problem assembles and factors S (block-6 Cholesky), then a wave per column of Sigma_OO, a wave per camera, a thread per pair entry, each phase a launch
 * of its own -- data crosses workgroups only at launch boundaries.  The pair kernel of csrc/pose_cov.hip propagates, as for the other entries. */
#define SUO_POSE_COV_GRAPH_MAX_OBJ 64
int suo_pose_covariances_graph(const suo_ba_problem* problem, int n_pair, const int32_t* pair_a, const int32_t* pair_b, double* cam_cov /*[n_cam][36]*/,
                               double* obj_cov /*[n_obj][36]*/, double* cross /*[n_pair][36]*/, double* rel /*[n_pair][36]*/,
                               int* status /*[3]: NaN cam blocks, NaN obj blocks, NaN pairs*/);
int suo_pose_covariances_graph_batch(const suo_ba_problem* problems, int n, const int* n_pair, const int32_t* const* pair_a, const int32_t* const* pair_b,
                                     double* const* cam_cov, double* const* obj_cov, double* const* cross, double* const* rel, int* status /*[n][3]*/);

/* ---- per-edge leverages, studentised residuals and the chi2 scale ------------------------------------------------------------------
 * What the covariances above leave open: by how much the adjustment itself says they are too small or too large (the chi2 scale s0^2, which they do not apply),
 * and which measurements carry the misfit.  The state, the Hessian, the perturbation, the vertex coding and the NaN rules are those of suo_pose_covariances_graph.
 *   Counted.     An edge is counted when edge_inlier == 1 and its camera and object are not both fixed: the edges H is summed over.
 *   v_e          = uv - pi(T_c T_o p), the residual.
 *   J_e          = [J_c J_o], the 2x12 Jacobian in the [omega, upsilon] left-update convention of csrc/lm_device.h, with zero columns for a fixed vertex.
 *   Omega_e      from edge_info.
 *   Sigma_e      the joint 12x12 of the edge's two vertices, cut out of Sigma = H^-1: [[Sigma_cc, Sigma_co], [Sigma_oc, Sigma_oo]].
 * For EVERY edge, counted or not:
 *   chi2_e       = v_e^T Omega_e v_e, with no Huber weight.
 *   P_e          = J_e Sigma_e J_e^T, the covariance of the predicted measurement, reported as (xx, xy, yy).
 *   lev_e        = tr(P_e Omega_e), the leverage.  For counted edges 0 <= lev_e <= 2 and 2 - lev_e is the edge's redundancy; over the counted edges of a problem
 *                sum lev_e = n exactly, n the number of rows of H (six per free vertex that a counted edge reaches): this is tr(Sigma H).
 *   t_e          = v_e^T (Omega_e^-1 + s P_e)^-1 v_e, s = -1 for a counted edge and s = +1 otherwise: the studentised statistic, chi2(2) under the model, of a
 *                measurement inside the estimate (its residual has covariance Omega^-1 - P) or outside it (Omega^-1 + P).  An edge with both vertices fixed has
 *                P_e = 0, so t_e = chi2_e, to the bit.
 *   No redundancy.  Let R_e = I + s P_e Omega_e (so that t_e = (Omega_e v_e)^T R_e^-1 v_e).  If det R_e <= 1e-9, or a diagonal entry of R_e is <= 0, then t_e is NaN
 *                and the edge is counted in status[3]: such an edge cannot be checked -- an object held by exactly three keypoints in a single-view frame is an
 *                example.  chi2_e, P_e and lev_e are still reported.  The threshold is part of the rule, not a tolerance.
 *   NaN vertex.  If either vertex of an edge is NaN in the marginal call, P_e, lev_e and t_e are NaN and the edge is counted in status[2]; chi2_e is still finite.
 * Per vertex, over its counted edges in ascending edge index: (count, sum chi2_e, sum (2 - lev_e)); the ratio of the last two is a per-vertex variance component.
 * Per problem, summary[6]: m (counted edges), n, sum chi2_e, sum lev_e, dof = 2 m - n, s0^2 = sum chi2_e / dof -- NaN when dof <= 0 or when any counted edge is NaN
 * (status[2]).  The sums run over the counted edges in ascending edge index in a tree whose shape depends on n_edge alone.
 * s0^2 is the factor by which the reported covariances would be multiplied to agree with the residuals; no entry of this library applies it (the pose NEES of
 * suo_pose_nees is measured under whatever covariance the caller hands it).
 * Host buffers, blocking, staged through the arena of suo_optimize_batch; the problem is not modified.  Every output pointer may be NULL:
 *   cam_cov [n_cam][36], obj_cov [n_obj][36]   those of suo_pose_covariances_graph on the same problem, bit for bit, as are status[0..1]
 *   edge_chi2 [E], edge_pcov [E][3], edge_lev [E], edge_t [E]      in the caller's edge order
 *   cam_stat [n_cam][3], obj_stat [n_obj][3]
 *   summary [6], status [4] = NaN camera blocks, NaN object blocks, NaN edges, edges without redundancy
 * It accepts what suo_pose_covariances_graph accepts (every form, up to SUO_POSE_COV_GRAPH_MAX_OBJ free objects next to free cameras) and refuses what it refuses,
 * SUO_ERR_ARG and nothing launched.  n_edge == 0 is legal: summary = {0, 0, 0, 0, 0, NaN}, cam_cov / obj_cov what the graph entry gives.  The batch form takes one
 * pointer per problem, summary [n][6] and status [n][4]; a problem's outputs do not depend on the rest of the batch, and two calls give the same bits.
 * Kernels: the graph entry's, asked for the cross blocks of the distinct (camera, object) pairs that carry an edge, then csrc/resid_stats.hip behind them (fp64, fixed
 * summation order, vector stores only, no atomics): a thread per edge, the three 6x6 blocks of a pair staged once per wave in LDS; then a wave per vertex for the
 * per-vertex triples (a fixed tree over the vertex's ascending edge list) and one workgroup per problem for the summary. */
int suo_residual_statistics(const suo_ba_problem* problem, double* cam_cov /*[n_cam][36]*/, double* obj_cov /*[n_obj][36]*/, double* edge_chi2 /*[E]*/,
                            double* edge_pcov /*[E][3]*/, double* edge_lev /*[E]*/, double* edge_t /*[E]*/, double* cam_stat /*[n_cam][3]*/,
                            double* obj_stat /*[n_obj][3]*/, double* summary /*[6]*/, int* status /*[4]*/);
int suo_residual_statistics_batch(const suo_ba_problem* problems, int n, double* const* cam_cov, double* const* obj_cov, double* const* edge_chi2,
                                  double* const* edge_pcov, double* const* edge_lev, double* const* edge_t, double* const* cam_stat, double* const* obj_stat,
                                  double* summary /*[n][6]*/, int* status /*[n][4]*/);

/* ---- covariance of a tracked camera with the map's uncertainty carried in ------------------------------------------------------------
 * For the camera-tracking graph (every object fixed at its map pose) suo_pose_covariances reports Hcc^-1: the covariance of a camera tracked against a perfectly
 * known map.  The map has a covariance of its own, Sigma_OO (suo_pose_covariances_graph reports it), and the tracker does not estimate it: it "considers" it.
 * The covariance of what the tracker actually computes is the Schmidt consider covariance
 *     P_c = Hcc^-1 + G Sigma_OO G^T,    G = Hcc^-1 [B_c1 ... B_cn],    B_co = sum over the counted edges e of (c, o) of J_c^T Omega J_o
 * with the Jacobians, the perturbation (left update exp(delta) * T, delta = [omega, upsilon]) and Ad(T) of the blocks above.
 *   Problem.     Every object is fixed; a free object is SUO_ERR_ARG and nothing is launched.  Any number of cameras: they are independent of each other here.
 *                n_obj <= SUO_POSE_COV_GRAPH_MAX_OBJ; more is SUO_ERR_ARG naming the count.
 *   map_cov      [6 n_obj][6 n_obj] row-major: the covariance of the stacked object perturbations in the problem's object order -- the objects' diagonal blocks and
 *                (object a, object b) cross blocks of suo_pose_covariances_graph.  Only the upper triangle with the diagonal is read, and mirrored; the lower
 *                triangle is ignored.  An object whose diagonal block has NaN at its (0, 0) entry is "not in the map": its edges are not counted, its cross and rel
 *                blocks are 36 NaNs, no other entry of its rows and columns is read, and status[1] counts it.  An object first initialised from this very view is
 *                not independent of the view's measurements and is excluded this way.  map_cov must not contain the measurements of the problem's own edges.
 *   Counted.     An edge is counted when edge_inlier == 1, its camera is free and its object is in the map.  No Huber weight, no lambda.
 * Per camera c, every block 36 row-major doubles:
 *   fixed_map_cov [n_cam][36]         Hcc^-1.  With every object in the map this is cam_cov of suo_pose_covariances on the same problem, bit for bit.
 *   cam_cov       [n_cam][36]         P_c, exactly symmetric.
 *   cross         [n_cam][n_obj][36]  Sigma_co = -(G Sigma_OO)[:, o]: rows are the camera, columns the object.  Dense: also for objects the camera does not see.
 *   rel           [n_cam][n_obj][36]  the covariance of T_OtoC = T_c T_o:  P_c + A Sigma_oo A^T + Sigma_co A^T + A Sigma_oc,  A = Ad(T_c).  Exactly symmetric.
 *   - A fixed camera: cam_cov, fixed_map_cov and cross are zeros and rel = A Sigma_oo A^T.
 *   - A free camera without a counted edge, or whose Hcc meets a non-positive pivot: every block of that camera is NaN; status[0] counts such cameras.  The call
 *     never faults and never loops on one.
 *   - The chi2 scale is not applied.
 * Host buffers, blocking, staged through the arena of suo_optimize_batch; the problem is not modified.  Every output pointer may be NULL.  status [2] = NaN cameras,
 * objects not in the map.  The batch form takes one pointer per problem and status [n][2]; a problem's bits do not depend on the rest of the batch, and two calls give
 * the same bits.  Kernels (fp64, fixed summation order, vector stores only, no atomics): Hcc^-1 by the camera form of csrc/pose_cov.hip; then csrc/track_cov.hip,
 * one workgroup per (problem, camera): a thread per object sums B_co over the pair's edges in ascending edge index, G (6 x 6 n_obj) lives in LDS, Z = G Sigma_OO is
 * a thread per column accumulating in ascending row of Sigma_OO, which is read once per camera from device memory, Z G^T is a fixed tree per entry; cross is -Z
 * written out and rel follows per object. */
int suo_tracking_covariances(const suo_ba_problem* problem, const double* map_cov /*[6 n_obj][6 n_obj]*/, double* cam_cov /*[n_cam][36]*/,
                             double* fixed_map_cov /*[n_cam][36]*/, double* cross /*[n_cam][n_obj][36]*/, double* rel /*[n_cam][n_obj][36]*/,
                             int* status /*[2]: NaN cameras, objects not in the map*/);
int suo_tracking_covariances_batch(const suo_ba_problem* problems, int n, const double* const* map_cov, double* const* cam_cov, double* const* fixed_map_cov,
                                   double* const* cross, double* const* rel, int* status /*[n][2]*/);

/* ---- phase-wise bundle adjustment for the multi-GPU global pose graph ------------------------
 * Cameras are partitioned across GPUs; each rank builds a context over ITS cameras' edges and ALL objects, and
 * a host driver (suo_slam_amd/ba_dist.py) runs g2o's LM schedule with two all-reduces per trial (RCCL):
 *   suo_ba_linearize   -> [chi2_local | (Hoo 21 + bo 6) per object | max diag Hcc]         (sum / max over ranks)
 *   suo_ba_schur       -> [S_g (ns x ns) | r_g (ns) | ok]   S_g = sum_c Hco^T (Hcc + lambda I)^-1 Hco  (sum)
 *   suo_ba_solve_update(in = [Hoo+bo totals | S_total | r_total]) -> [chi2_local | scale_cams | scale_objs | ok]
 *   suo_ba_restore      = pop() after a rejected trial;  suo_ba_classify = chi2 re-classification of own edges.
 * ns = 6 * (#free objects); beyond 96 rows (16 free objects) the reduced system is factorised in global memory. */
typedef struct suo_ba_ctx suo_ba_ctx;
int suo_ba_ctx_create(suo_ba_problem* local_problem, suo_ba_ctx** out);
void suo_ba_ctx_destroy(suo_ba_ctx* ctx);
int suo_ba_ctx_ns(const suo_ba_ctx* ctx);
int suo_ba_classify(suo_ba_ctx* ctx, int keep_all, double* num_good_local);
int suo_ba_linearize(suo_ba_ctx* ctx, int robust_on, double* out);
int suo_ba_schur(suo_ba_ctx* ctx, double lambda, double* out);
int suo_ba_solve_update(suo_ba_ctx* ctx, double lambda, int robust_on, const double* in, double* out);
int suo_ba_restore(suo_ba_ctx* ctx);
int suo_ba_ctx_download(suo_ba_ctx* ctx, suo_ba_problem* local_problem);
/* The same phases on caller-owned DEVICE buffers: stream-ordered on `stream` (the caller's, e.g. the one RCCL orders its
 * collectives against), no host synchronisation, nothing staged through host memory -- the buffers are all-reduced in place.
 *   lin_dev [1 + 27 n_obj + world] = [chi2_local | (Hoo 21 + bo 6) per object | max |diag Hcc| in slot `rank`, 0 elsewhere]  (SUM)
 *   sch_dev [ns*ns + ns + 1]       = [S_g | r_g | ok]                                                                    (SUM)
 *   red_dev [4]                    = [chi2_local | scale over own cameras | ok | scale over objects (identical on every rank)]
 *                                    (SUM over the first three)
 * suo_ba_solve_update_dev takes the REDUCED lin_dev / sch_dev and treats the trial as failed unless sch_dev's ok count == world.
 * Before suo_ba_ctx_download the caller synchronises `stream`. */
int suo_ba_classify_dev(suo_ba_ctx* ctx, int keep_all, double* num_good_dev, void* stream);
int suo_ba_linearize_dev(suo_ba_ctx* ctx, int robust_on, int rank, int world, double* lin_dev, void* stream);
int suo_ba_schur_dev(suo_ba_ctx* ctx, double lambda, double* sch_dev, void* stream);
int suo_ba_solve_update_dev(suo_ba_ctx* ctx, double lambda, int robust_on, int world, const double* lin_dev, const double* sch_dev,
                            double* red_dev, void* stream);
int suo_ba_restore_dev(suo_ba_ctx* ctx, void* stream);
/* The same phases under a DEVICE-RESIDENT LM schedule: g2o's accept / reject arithmetic (optimization_algorithm_levenberg.cpp:88-148) runs in
 * one-thread kernels on the reduced scalars and keeps its state in ctl_dev [16 doubles]:
 *   [0] lambda [1] ni [2] current chi2 [3] state (0: the next unit linearises, 1: the next unit is a trial on the standing linearisation,
 *   2: the round is over) [4] iterations done this round [5] iteration budget [6] qmax [7] LM iterations [8] LM trials (all rounds; zero them
 *   once) [9] rho [10] restore flag [11] ranks.
 * One UNIT = suo_ba_lm_linearize_dev (live in state 0; always leaves this rank's totals in lin_dev) -> all-reduce(lin_dev) ->
 * suo_ba_lm_schur_dev (chi2 / lambda init of a fresh linearisation, then the Schur phase for ctl's lambda) -> all-reduce(sch_dev) ->
 * suo_ba_lm_solve_update_dev -> all-reduce(red_dev[0:3]) -> suo_ba_lm_decide_dev (gain ratio, lambda / ni, restore of a rejected step,
 * next state).  Phases that are not live return at once, so units may be enqueued blindly -- the host reads ctl_dev once per batch of
 * units instead of four doubles per trial (suo_slam_amd/ba_dist.py: optimize_distributed).  suo_ba_lm_begin_dev starts a round of `its`
 * iterations (optimizer.optimize(its), lib/object_slam.py:873-875). */
int suo_ba_lm_begin_dev(suo_ba_ctx* ctx, double* ctl_dev, int its, int world, void* stream);
int suo_ba_lm_linearize_dev(suo_ba_ctx* ctx, int robust_on, int rank, int world, const double* ctl_dev, double* lin_local_dev, double* lin_dev,
                            void* stream);
int suo_ba_lm_schur_dev(suo_ba_ctx* ctx, double* ctl_dev, const double* lin_dev, double* sch_dev, void* stream);
int suo_ba_lm_solve_update_dev(suo_ba_ctx* ctx, int robust_on, int world, const double* ctl_dev, const double* lin_dev, const double* sch_dev,
                               double* red_dev, void* stream);
int suo_ba_lm_decide_dev(suo_ba_ctx* ctx, double* ctl_dev, const double* red_dev, void* stream);
/* The same unit on ONE rank, where nothing is exchanged between its phases: one call, the control steps folded into the kernels in front of them (12 launches
 * instead of 14), bit-identical to the four calls above back to back. */
int suo_ba_lm_unit_one_rank_dev(suo_ba_ctx* ctx, int robust_on, double* ctl_dev, double* lin_local_dev, double* lin_dev, double* sch_dev, double* red_dev, void* stream);
/* Test entry (finite-difference checks of what the KERNELS linearise, not of the oracle): after suo_ba_linearize, per edge in
 * the caller's order jac_out[e][29] = [J_cam 2x6 | J_obj 2x6 | w*info (xx,xy,yy) | -w*info*err (2)] (EdgeSE3ProjectFromObject::
 * linearizeOplus, types_object_slam.cpp:70-123, columns = [omega, upsilon]) and err_out[e][2] (computeError, :45-60). */
int suo_debug_ba_jacobians(suo_ba_ctx* ctx, int n_edge, double* jac_out, double* err_out);
/* Test entry: the reduced (object) system's solve as the LM kernels run it -- block-6 Cholesky of one workgroup, trailing updates on v_mfma_f64_16x16x4_f64 tiles, the
 * right-hand side eliminated inside the factorisation (csrc/lm_device.h: wg_cholesky_solve; g2o solves the same system with a sparse LL^T, block_solver.hpp:464-566 /
 * linear_solver_cholmod.h) -- on a dense symmetric A [ns][ns] (HOST, row-major, lower triangle read; ns a multiple of 6, at most 96) and b [ns]: x_out [ns] solves
 * A x = b; *ok_out = 0 when a pivot was not positive (the LM kernels then reject the trial). */
int suo_debug_cholesky_solve(const double* A, const double* b, int ns, double* x_out, int* ok_out);
/* Test entry: the SE(3) update every LM kernel applies to a vertex, through the very pose_from_T, pose_oplus and pose_to_T of csrc/lm_device.h (VertexSE3Expmap::
 * oplusImpl, types_six_dof_expmap.h:100-103; SE3Quat::exp and operator*, se3quat.h:220-254, :101-114).  HOST arrays, blocking, one launch, one thread per pose:
 * T_in [n][12] row-major 3x4 (R | t), u [n][6] = (omega, upsilon), T_out [n][12] = exp(u) * T_in -- the LEFT update: R' = exp(omega^) R, t' = V(omega) upsilon +
 * exp(omega^) t -- and, unless q_out is NULL, q_out [n][4]: the unit quaternion (w, x, y, z; w >= 0) the kernels keep after the update, of which T_out's rotation is
 * the matrix.  The input rotation goes through the Eigen matrix-to-quaternion conversion first (trace > 0: one form; else one of three pivot forms), as when a
 * problem is loaded.  Coefficients of exp, with th2 = |omega|^2:
 *   th2 < 1e-10   g2o's shortcut R = V = I + Om + Om^2 (se3quat.h:236-240; not a rotation to second order: the quaternion conversion normalises it);
 *   th2 < 0.09    eight-term Taylor series in th2 of sin(th) / th, (1 - cos(th)) / th^2, (th - sin(th)) / th^3;
 *   else          those closed forms.
 * n <= 0 or a NULL T_in, u or T_out: SUO_ERR_ARG, nothing launched. */
int suo_debug_pose_oplus(const double* T_in, const double* u, int n, double* T_out, double* q_out);
/* Test entry: the refinement half of the PnP kernel (PNP::refine, pnp_ransac.cpp:240-326) on its own, through the very device functions pnp_batch_kernel calls
 * (csrc/pnp.hip: p4p, count_inliers, select_inliers, refine_normal_eqs, refine_cost, refine_pass, refine_sequence).  HOST arrays, blocking, one launch, one wave per
 * object; objects are ragged as in suo_pnp_batch: n_pts [n_obj], xs [sum n][3], ys [sum n][2] (normalised), sel_in / sel0_out / sel1_out [sum n] in the same order.
 * Per object o:
 *   start      start_idx[o][4] with [0] >= 0: the start is p4p of those four points; else start_qt[o][7] = (q w x y z, t), used as given
 *   mode[o]    0 SEQUENCE: select, refine 5 iterations at 1e-6, reselect, 3 iterations at 1e-8 unless deltas < 0.05 m -- what suo_pnp_batch runs with do_refine
 *              1 PASS: one refine pass of max_iter[o] (0 .. 50) iterations at tolerance tol[o] over the points with sel_in != 0
 *   out_d[o][88]  [0:7] the start (q, t) used  [7:43] H = J'J row-major and [43:49] g = J'r and [49] cost = 1/2 sum |r|^2, all at the start over the first
 *              selection (columns: the three local coordinates of Ceres' QuaternionParameterization, then t)  [50:57] (q, t) after the first pass  [57:64] the final
 *              (q, t)  [64:76] the pose after the first pass as row-major 3x4  [76:88] the final pose as 3x4.  PASS: final = after the pass.
 *   out_i[o][8]   [0] inliers of the start by the RANSAC count rule (1 / z < 0 skips, err < thr^2 counts)  [1] m0, size of the first selection  [2] m1, size of the
 *              reselection  [3] deltas, flags that changed  [4] 1 when the second pass ran  [5:8] 0.  PASS: m1 = deltas = [4] = 0.
 *   sel0_out, sel1_out   the two selections as 0 / 1 per point by the refinement's rule (z < 0 drops, err > thr^2 drops); PASS: sel0 = sel_in != 0, sel1 = 0.
 * Refused with SUO_ERR_ARG, nothing launched, nothing written: n_obj <= 0, a NULL pointer, n_pts[o] < 0 or > 1024, a start index outside [0, n_pts[o]), a mode
 * other than 0 / 1, max_iter outside 0 .. 50 on a PASS object. */
int suo_debug_pnp_refine(int n_obj, const int* n_pts, const double* xs, const double* ys, double threshold, const int* mode, const double* start_qt,
                         const int* start_idx, const int* sel_in, const int* max_iter, const double* tol, double* out_d, int* out_i, int* sel0_out,
                         int* sel1_out);
/* Test entry: the minimal solver every lane of the PnP kernel runs per hypothesis (p3p_lambdatwist<double,5>, lambdatwist/lambdatwist.p3p.h; p4p, p4p.cpp:11-60),
 * through the very p3p_lambdatwist and p4p of csrc/pnp.hip.  HOST arrays, blocking, one launch, one thread per problem in 64-thread workgroups.  A problem is four
 * points: xs [n][4][3] model points, ys [n][4][2] normalised image points.  Per problem i:
 *   valid[i]      the number of candidates p3p_lambdatwist returned for points 0, 1, 2 (0 .. 4)
 *   R[i][4][9]    its rotations, row-major, and t[i][4][3] its translations, in its order, exactly as it wrote them; zero beyond valid[i]
 *   qt[i][7]      (q w x y z, t) as p4p(xs, ys, {0, 1, 2, 3}) returned it: the candidate with the smallest reprojection error of point 3 among those that put it at
 *                 z >= 0 (strictly smaller: the first of equals wins), the identity pose when none survives
 *   status[i]     1 when qt[i] is the identity pose (1, 0, 0, 0, 0, 0, 0) exactly, else 0
 * Inputs are not screened: degenerate triples, equal bearings and NaN coordinates are the solver's to handle.
 * Refused with SUO_ERR_ARG, nothing launched, nothing written: n <= 0, a NULL pointer. */
int suo_debug_p3p(int n, const double* xs, const double* ys, int* valid, double* R, double* t, double* qt, int* status);
/* Test entry: the pose graph fg_prep_kernel and fg_build_kernel (csrc/frame_geom.hip) staged on the device in the context's last suo_frame_geom_launch, as the LM
 * kernel read it.  Waits for that launch, then copies the device arrays to HOST buffers, blocking; any output pointer may be NULL.  L = crops of the launch,
 * F = its frames, SLOT layout: crop l owns slots l * 41 .. l * 41 + 40 and fills the first n_kp[l] of them with its valid keypoints in mask order; the slots behind
 * them are not written by the launch (they hold what an earlier launch of the context left, zeros in a fresh one).
 *   xs [L][41][3] model points, ys [L][41][2] normalised image points (the PnP problem), edge_uv [L][41][2] measurements, edge_k [L][41][4] fx, fy, cx, cy,
 *   edge_info [L][41][3] (xx, xy, yy), pair_start / pair_end [L] edge range of the crop's pair relative to its FRAME's first slot (start = lane * 41, end = start +
 *   n_kp for an accepted crop, = start for a rejected one), obj_fixed [L] = !accepted, problem_header [F][4] = n_cam, n_obj, n_edge, n_pair of each frame's LmProblem.
 * SUO_ERR_ARG when nothing was launched. */
int suo_debug_frame_geom_staged(suo_frame_geom* g, double* xs, double* ys, double* edge_uv, double* edge_k, double* edge_info, int* pair_start, int* pair_end,
                                unsigned char* obj_fixed, int* problem_header);

/* ---- the partitioned adjustment driven from C (csrc/ba_comm.hip, csrc/ba_drive.hip: optimize_dist) ---------------------------------
 * suo_ba_comm: the one collective the schedule above needs -- an in-place SUM all-reduce of n doubles on a device buffer, ordered on a stream.
 *   RCCL backend: one rank per process and device.  suo_ba_comm_rccl_unique_id fills the 128 bytes of an ncclUniqueId on ONE rank; the caller carries them to
 *     the others (any transport) and every rank calls suo_ba_comm_create_rccl on its current device.  ncclAllReduce(ncclDouble, ncclSum) on the driver's stream.
 *     RCCL is resolved at first use with dlopen (RTLD_LOCAL): a copy the process already holds (e.g. PyTorch's), else the path in SUO_RCCL_LIB (a path that does
 *     not load is an error, not a reason to look further), else librccl.so.1 on the loader path.  No RCCL: SUO_ERR_MISSING and a message, never an abort.
 *   local backend: suo_ba_comm_create_local(world): `world` (1..16) ranks inside ONE process on ONE device and ONE stream.  The ranks' exchange buffers lie
 *     `stride` doubles apart in one device block and the all-reduce is one launch of ba_local_allreduce_kernel: every element's addends summed in fp64 in ASCENDING
 *     RANK ORDER, ((b0 + b1) + b2) + ..., written back to all `world` slots; no atomics, no second pass.  It runs the N-rank SCHEDULE on one GPU -- to test it and
 *     to check a partitioning -- and is slower than suo_optimize by construction (world x the launches on one stream).
 * suo_ba_comm_allreduce: buf_dev = this rank's buffer (local backend: rank 0's; rank r's is buf_dev + r * stride, stride >= n; RCCL ignores stride).
 * suo_ba_comm_calls: all-reduces issued through the communicator so far. */
typedef struct suo_ba_comm suo_ba_comm;
int suo_ba_comm_rccl_unique_id(void* id128);
int suo_ba_comm_create_rccl(const void* id128, int rank, int world, suo_ba_comm** out);
int suo_ba_comm_create_local(int world, suo_ba_comm** out);
void suo_ba_comm_destroy(suo_ba_comm* comm);
int suo_ba_comm_rank(const suo_ba_comm* comm);
int suo_ba_comm_world(const suo_ba_comm* comm);
uint64_t suo_ba_comm_calls(const suo_ba_comm* comm);
int suo_ba_comm_allreduce(suo_ba_comm* comm, double* buf_dev, size_t stride, size_t n, void* stream);
/* Test entry: the local backend's kernel on a caller-owned block (slot r = block_dev + r * stride; the doubles between n and stride are not touched).
 * 16-byte loads / stores when block_dev is 16-byte aligned and stride is even, scalar otherwise.  stream NULL: the null stream, blocking. */
int suo_debug_ba_local_allreduce(double* block_dev, int world, size_t stride, size_t n, void* stream);
/* optimize_distributed of suo_slam_amd/ba_dist.py as one C call.  Every rank passes the same FULL problem and gets the complete result back in it (cam_T, obj_T,
 * inlier flags, chi2, stats).  Cameras are dealt round-robin (camera c to rank c % world; suo_ba_split), every rank keeps all objects; per LM iteration one
 * all-reduce (linearisation totals), per LM trial two ([S | r | ok], three step scalars), one per classification, one for the result assembly.  Eager launches
 * on one internal stream, the device-resident accept / reject schedule, a look at the control block once per suo_ba_units_per_look(world) units.
 * With a local communicator the call runs all `world` ranks itself, phase by phase, and returns the one result; suo_optimize_partitioned(p, n) is that with a
 * communicator of its own.  A rank without a camera (world > n_cam) takes part in every collective with zeros. */
int suo_optimize_dist(suo_ba_problem* full, suo_ba_comm* comm);
int suo_optimize_partitioned(suo_ba_problem* problem, int n_parts);
/* Host only: rank `rank`'s share.  cams_out [<= n_cam]: its cameras, ascending (local camera index = position); edges_out [<= n_edge]: its edges in the
 * caller's order (suo_slam_amd/ba_dist.py: split_problem). */
int suo_ba_split(const suo_ba_problem* full, int rank, int world, int* cams_out, int* n_cams, int* edges_out, int* n_edges);
/* units enqueued between two looks at the control block: 12 on one rank, 6 on several (a dead unit there costs three all-reduces) */
int suo_ba_units_per_look(int world);

/* ---- evaluation meter: ADD / ADD-S pose errors ------------------------------------
 * Replaces the distance part of EvalMeter.update (lib/utils/eval_meter.py:126-155,233-242):
 *   ADD = mean_i |T_gt p_i - T_pred p_i|,  ADD-S = mean_i min_j |T_gt p_i - T_pred p_j|   (fp32, mesh units = mm).
 * suo_mesh_db_create uploads the model point clouds once (mesh_db[obj]["points"], lib/utils/mesh_database.py:31-40):
 * n_pts[n_models], pts = the clouds concatenated, [sum(n_pts)][3] floats, host memory.
 * suo_pose_errors evaluates n (model, pose pair) items in one launch set: model_index[n] into the database,
 * T_pred / T_gt [n][12] = row-major 3x4 [R|t] (host), results add[n], adds[n] (host).  Blocking. */
int suo_mesh_db_create(int n_models, const int* n_pts, const float* pts, void** mesh_db_out);
void suo_mesh_db_destroy(void* mesh_db);
int suo_pose_errors(void* mesh_db, int n, const int* model_index, const float* T_pred, const float* T_gt, float* add, float* adds);

/* ---- BOP-19 MSSD / MSPD pose errors --------------------------------------------------
 * Replaces bop_toolkit_lib/pose_error.py:96-144 (mssd, mspd; misc.py:93-107 project_pts, misc.py:266-276 transform_pts_Rt) over the same mesh database.
 * For every symmetry transformation s = [S_R|S_t] of the model:  R_s = R_gt S_R,  t_s = R_gt S_t + t_gt,
 *   MSSD = min_s max_i |(R_est p_i + t_est) - (R_s p_i + t_s)|                 (mm)
 *   MSPD = min_s max_i |pi(K, R_est, t_est, p_i) - pi(K, R_s, t_s, p_i)|       (px),  pi = (K X)_xy / (K X)_z, divided as given: a point behind the
 *                                                                                camera keeps its finite value, as in the toolkit.
 * All arithmetic is fp64 (the toolkit's; the recall compares these errors with thresholds) on the float32 points widened exactly.  max and min are exact and
 * a (symmetry, point) value does not depend on the launch shape, so a pair in a batch has the bits it has alone.  One stated deviation: a pair that meets a
 * non-finite projection or distance (z exactly 0, a NaN pose) reports +inf for that metric -- the toolkit's min() over NaNs depends on their order.
 * suo_mesh_db_set_symmetries: symmetry transformations per model of an existing mesh database: n_sym[n_models] (each >= 1; the identity is one of them and
 * is the caller's to list), sym [sum n_sym][12] row-major 3x4 [R|t], host doubles; replaces an earlier set.  Without this call every model has the identity alone.
 * suo_pose_errors_bop: n (estimate, ground truth) pairs: model_index[n], T_est / T_gt [n][12] row-major 3x4 (doubles, mm), K [n][9] row-major (may be NULL
 * when mspd is).  mssd[n] (mm), mspd[n] (px); either output may be NULL.  Host buffers, blocking.  n = 0 returns 0.
 * SUO_ERR_ARG (nothing launched): a null database or required pointer, n < 0, a model index outside the database, n_sym[i] < 1. */
int suo_mesh_db_set_symmetries(void* mesh_db, const int* n_sym, const double* sym);
int suo_pose_errors_bop(void* mesh_db, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, double* mssd, double* mspd);

/* ---- consistency of the reported uncertainties: pose NEES and keypoint chi2 ------------------------------------------------------
 * Compares a reported covariance with ground truth: the normalised estimation error squared of a pose under its 6x6 covariance (suo_pose_covariances,
 * suo_pose_covariances_pairs' `rel`) and the chi2 of a keypoint's reprojection error under the network's 2x2 covariance.  fp64, no contraction, fixed summation
 * order: two calls give the same bits and a pair in a batch has the bits it has alone.
 *
 * suo_pose_nees: n (estimate, ground truth, covariance) triples over the mesh database and its symmetry sets (suo_mesh_db_set_symmetries).
 *   Symmetry.    s* = the symmetry that attains the MSSD minimum min_s max_i |T_est p_i - T_gt S_s p_i| (the per-symmetry maxima of suo_pose_errors_bop's own
 *                kernel).  On equal maxima the LOWEST index wins.  sym_index[i] = s*, an index into the model's set.
 *   Reference.   T_ref = T_gt S_s*:  R_ref = R_gt S_R,  t_ref = R_gt S_t + t_gt, as above.
 *   Error.       xi = log(T_est T_ref^-1) = [omega, upsilon]: the inverse of the library's update T <- exp([omega, upsilon]) T (csrc/lm_device.h, g2o's
 *                SE3Quat::exp), the perturbation the covariances above are defined for -- not a free choice.  omega = 2 atan2(|v|, w) v / |v| from the unit
 *                quaternion (w >= 0, v) of R_est R_ref^T; upsilon = V^-1 t, V = I + b Om + c Om^2 of the exponential.  Series for atan2(|v|, w) / |v| below
 *                |v|^2 < 1e-8 and for the V^-1 coefficient below theta^2 < 0.09, closed forms above.  Covered: 0 <= theta <= 3.0 rad to a few ulp of
 *                (1 + |xi|); beyond 3.0 only finiteness and |omega| <= pi are promised.
 *   NEES.        xi^T Sigma^-1 xi through the Cholesky factor of Sigma (cov [n][36] row-major, rows and columns [omega, upsilon]; the lower triangle is read).
 *                The chi2 scale is STILL NOT applied: this is the NEES under the covariance the caller hands over -- the unscaled one, unless the caller has
 *                multiplied it by the s0^2 that suo_residual_statistics reports.
 *   NaN rules.   nees[i] is NaN for a block with a non-finite entry (all 36 are looked at), for a pivot that is not positive (this includes the 36 zeros of a
 *                fixed vertex), and for a pair whose MSSD meets a non-finite distance (a NaN or overflowing pose): that pair also gets sym_index -1 and NaN xi
 *                and T_ref.  status[0] counts the NaN results.  The call never faults and never loops on a bad block; the other pairs of the batch are unaffected.
 *   Units.       Poses, symmetry translations, mesh points and the upsilon rows and columns of cov share ONE length unit (mm throughout this project's evaluation;
 *                the rotation rows are radians).
 *   Outputs.     nees [n]; xi [n][6], sym_index [n], T_ref [n][12] row-major 3x4, status [1]: each may be NULL.
 *
 * suo_keypoint_nees: ragged over n_det detections like suo_pnp_batch: n_pts[n_det] keypoints each (0 is fine), model_kp / uv / cov concatenated in that order
 * (cov row-major 2x2), K [n_det][9] row-major (the K_bbox of the crop the uv live in), T_ref [n_det][12] (e.g. suo_pose_nees' T_ref).  Per keypoint:
 *   e    = uv - pi(K, T_ref x),  pi = (K X)_xy / (K X)_z divided as given: a point behind the camera keeps its finite value;
 *   chi2 = e^T C^-1 e by the closed 2x2 inverse; NaN when det C <= 0, when a diagonal entry is not positive, or when an input (or the result) is not finite.
 *   chi2 [sum n_pts]; err [sum n_pts][2] (= e) may be NULL.  The mesh database lends its scratch and stream only.
 * Host buffers, blocking, staged through the database's grow-only scratch.  n = 0 / n_det = 0 return 0.  SUO_ERR_ARG with a message and nothing launched: a null
 * database, a null required pointer, n < 0 / n_det < 0, a model index outside the database, a negative n_pts.  Kernels: csrc/eval_nees.hip (one pair per 8-lane
 * group; one thread per keypoint). */
int suo_pose_nees(void* mesh_db, int n, const int* model_index, const double* T_est /*[n][12]*/, const double* T_gt /*[n][12]*/,
                  const double* cov /*[n][36] row-major, [omega, upsilon]*/, double* nees /*[n]*/, double* xi /*[n][6] or NULL*/,
                  int* sym_index /*[n] or NULL*/, double* T_ref /*[n][12] or NULL*/, int* status /*[1] or NULL*/);
int suo_keypoint_nees(void* mesh_db /*scratch + stream only*/, int n_det, const int* n_pts, const double* model_kp /*[sum][3]*/,
                      const double* uv /*[sum][2]*/, const double* cov /*[sum][4]*/, const double* K /*[n_det][9]*/,
                      const double* T_ref /*[n_det][12]*/, double* chi2 /*[sum]*/, double* err /*[sum][2] or NULL*/);

/* ---- BOP-19 VSD: depth rasteriser and error ------------------------------------------
 * The third term of the BOP-19 score over the same mesh database.  Opt-in: nothing above changes when these are not called.
 *
 * suo_mesh_db_set_faces: triangles per model, n_faces[n_models] (0 allowed: that model cannot be rendered), faces [sum n_faces][3] vertex indices into the
 * model's own point list, host ints; replaces an earlier set.  SUO_ERR_ARG, nothing uploaded: a null pointer, a negative count, an index outside [0, n_pts[i]).
 *
 * suo_render_depth: n depth images [n][height][width] (host floats, eye-space Z in the mesh's unit, 0.0f where nothing is drawn) of model_index[i] under the
 * pose T[i] (row-major 3x4 [R|t], doubles) and the camera K[i] (row-major 3x3; only fx = K[0], fy = K[4], cx = K[2], cy = K[5] are used, as in the toolkit's
 * Renderer.render_object).  It restates what bop_toolkit's Python renderer draws into its depth image (renderer_py.py:124-143, 185-226, 428-457, 524-556)
 * under OpenGL's rasterisation rules; no GL exists to pin it, so these rules ARE the specification (tests/vsd_ref.py restates them in fp64 numpy):
 *   camera space   X = R p + t in fp64 on the float32 points widened exactly, each row ((r0 x + r1 y) + r2 z) + t;  u = fx (X / Z) + cx,  v = fy (Y / Z) + cy.
 *   sample point   of pixel (x, y): (x + 0.5, y + 0.5).  This half pixel is the Python renderer's (its projection maps u to window x with x0 = y0 = 0 and GL
 *                  samples pixel centres; the y_down matrix plus the row flip after glReadPixels gives the same for rows) and is kept on purpose, although
 *                  the error below has none.
 *   coverage       fp64 edge functions on (u, v): E_PQ(p) = (Qx - Px)(py - Py) - (Qy - Py)(px - Px) for the edges 1->2, 2->0, 0->1, multiplied by the sign s of
 *                  the doubled area E_01(2) so that both windings are drawn (no face culling).  A sample is covered when all three are > 0, or == 0 on an edge
 *                  that is a left edge (inward normal s (-(Qy - Py), Qx - Px) has x > 0) or a top edge (x == 0 and y > 0; rows grow downwards).
 *                  Zero-area triangles are skipped.
 *   depth          eye-space Z, perspective-correct: 1 / z = ((w0 / Z0 + w1 / Z1) + w2 / Z2) / |area2| with the weights w_i = s E_i above (1 / Z_i rounded
 *                  once each); z is rounded once to float32.
 *   z-buffer       the nearest fragment wins (depth test "less"); the result does not depend on the order of the triangles or of the renders in a call.
 *   deviation      a triangle with any vertex at Z <= 0 is skipped whole (GL would clip it at a near plane placed at the nearest bounding-box corner, which
 *                  means nothing once that corner is behind the camera).
 * SUO_ERR_ARG before anything is launched: a null pointer, non-finite T or K, width or height < 1, a model index outside the database, a model without
 * faces, more than 65535 renders in a call.  n = 0 returns 0.  Blocking.
 *
 * suo_vsd_from_depth: the toolkit's pose_error.vsd (pose_error.py:40-93, cost 'step'; misc.py:130-163; visibility.py:9-75, mode 'bop19') operation for
 * operation on n pairs of rendered depth images depth_est / depth_gt [n][height][width] against the test depth image image_index[i] of depth_test
 * [n_images][height][width] (mm, host floats):  pre_X = (x - cx) / fx, pre_Y = (y - cy) / fy in fp64 (no half pixel: the toolkit has none),
 * dist = sqrt(((pre_X d)^2 + (pre_Y d)^2) + d^2) in fp64; the visibility differences in float32 on the distances rounded to float32, compared with
 * float32(delta); visib_gt = (diff_gt <= delta or dist_test == 0) and dist_gt > 0; visib_est = (the same for est) or (visib_gt and dist_est > 0);
 * cost_t = count over the intersection of |dist_gt - dist_est| (divided by diameter[i] when normalized_by_diameter) >= taus[t];
 * errors[i][t] = (cost_t + union - intersection) / union, or 1.0 when union == 0.  counts (may be NULL) [n][2 + n_taus]: union, intersection, cost per tau.
 * The counters are integers: they do not depend on the launch shape.  1 <= n_taus <= 16.
 * suo_pose_errors_vsd: the same on poses: renders T_est[i] and T_gt[i] of model_index[i] under K[i] on the device (each distinct (model, pose, fx, fy, cx, cy)
 * of the call once -- the ground truths repeat) and feeds the error kernel without the depth images leaving device memory.
 * SUO_ERR_ARG (nothing launched) as for suo_render_depth, and for an image index outside [0, n_images), n_taus outside 1..16, a non-finite delta. */
int suo_mesh_db_set_faces(void* mesh_db, const int* n_faces, const int* faces);
int suo_render_depth(void* mesh_db, int n, const int* model_index, const double* T, const double* K, int width, int height, float* depth_out);
int suo_vsd_from_depth(int n, int width, int height, const float* depth_est, const float* depth_gt, int n_images, const float* depth_test, const int* image_index,
                       const double* K, double delta, int n_taus, const double* taus, int normalized_by_diameter, const double* diameter, double* errors,
                       long long* counts);
int suo_pose_errors_vsd(void* mesh_db, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, int width, int height,
                        int n_images, const float* depth_test, const int* image_index, double delta, int n_taus, const double* taus, int normalized_by_diameter,
                        const double* diameter, double* errors, long long* counts);

/* ---- BOP scene_gt_info and ground-truth masks ------------------------------------------
 * What bop_toolkit's scripts/calc_gt_info.py:74-176 and scripts/calc_gt_masks.py:77-127 compute for n ground-truth instances: model_index[i] under the pose
 * T[i] and the camera K[i] (as for suo_render_depth) against the test depth image image_index[i] of depth_test [n_images][height][width] (mm, host floats).
 * Every entry is new; nothing above changes.
 *
 * suo_gt_info, per instance:
 *   render         on a canvas of 3 width x 3 height with the principal point (cx + width, cy + height), the sums formed on the host in fp64, under the rules
 *                  of suo_render_depth above, unchanged (the Z <= 0 deviation included).  depth_gt is the central width x height window of the canvas.  The
 *                  canvas exists tile by tile in LDS only; it is never written to memory.
 *   px_count_all   covered samples of the whole canvas.
 *   distances      over the window, for image pixel (x, y) and the ORIGINAL K, misc.depth_im_to_dist_im (misc.py:166-189; not the _fast form of the VSD error
 *                  above: the order of operations differs):  Xs = ((x - cx) d) (1 / fx),  Ys = ((y - cy) d) (1 / fy),  dist = sqrt((Xs^2 + Ys^2) + d^2), fp64
 *                  on the float32 depth widened exactly.
 *   visib          (float32(dist_gt) - float32(dist_test) <= float32(delta) or dist_test == 0) and dist_gt > 0        (visibility.py:9-42, mode 'bop19')
 *   px_count_valid pixels with dist_gt > 0 and dist_test > 0;   px_count_visib   pixels with visib.
 *   bbox_visib     [xmin, ymin, xmax - xmin, ymax - ymin] of visib: no + 1, no clipping (misc.calc_2d_bbox).
 *   bbox_obj       the same box of the covered samples of the whole canvas in image coordinates (canvas minus the offset): may be negative or exceed the image.
 *   both boxes     are [-1, -1, -1, -1] when px_count_visib == 0, also when px_count_all > 0 (calc_gt_info.py:155-166).
 *   px_counts      [n][3]: all, valid, visib.  visib_fract = px_count_visib / float(px_count_all), 0.0 when px_count_all == 0, is the caller's division.
 * suo_gt_masks: the same on the plain width x height canvas with (cx, cy), as calc_gt_masks.py renders: mask = 255 (dist_gt > 0), mask_visib = 255 visib, uint8
 * [n][height][width]; either may be NULL.
 * Test depth that is no measurement: a NaN gives a NaN distance -- not 0, so not "missing" -- and every comparison with it is false: the pixel is neither
 * valid nor visible.  A negative depth d has the distance of |d| (the squares lose the sign): the pixel is valid, and visible when dist_gt - that <= delta.
 * +-inf gives dist_test = inf (valid, and visible), or NaN where x == cx or y == cy (0 * inf).  The test image is read at window pixels only, whatever it holds.
 * The device writes integers only, reduced per wave, per workgroup and then by one integer atomic per quantity: the values of an instance do not depend on
 * the batch, its order or the tiling.  The rasterisation rule itself stays unpinned as in N6 (no GL here); everything after the render is pinned by the
 * toolkit's two scripts run unmodified over the numpy rasteriser (tests/golden/make_gt_info_golden.py).
 * Host buffers, blocking.  n = 0 returns 0.  SUO_ERR_ARG with a message, before anything is launched: as for suo_pose_errors_vsd (a null pointer, non-finite
 * T, K or delta, a model or image index out of range, a model without faces, width or height < 1), and a size whose canvas 3 width x 3 height exceeds what
 * the rasteriser's pixel boxes take (9 width height > 2^28).  More instances than one launch takes (1024, fewer with many triangles) are split inside. */
int suo_gt_info(void* mesh_db, int n, const int* model_index, const double* T, const double* K, int width, int height,
                int n_images, const float* depth_test, const int* image_index, double delta,
                long long* px_counts /*[n][3]: all, valid, visib*/, int* bbox_obj /*[n][4]*/, int* bbox_visib /*[n][4]*/);
int suo_gt_masks(void* mesh_db, int n, const int* model_index, const double* T, const double* K, int width, int height,
                 int n_images, const float* depth_test, const int* image_index, double delta,
                 uint8_t* mask /*[n][height][width], may be NULL*/, uint8_t* mask_visib /*may be NULL*/);

/* ---- model statistics: 3-D box and diameter ------------------------------------------
 * What bop_toolkit's scripts/calc_model_info.py computes for models_info.json (min_*, size_*, diameter; misc.py:279-293 calc_pts_diameter), for n items
 * model_index[i] of the mesh database, on its float32 points widened exactly to fp64.  Every entry is new; nothing above changes.
 *   box        min_c = min_i p_ic,  size_c = max_i p_ic - min_c: one fp64 subtraction.  -0 orders below +0: a zero minimum of an axis that holds both zeros
 *              is -0.0 (the toolkit's numpy reports whichever it meets first -- a stated deviation; size_c is the same number either way).
 *   diameter   d^2(i, j) = ((dx dx + dy dy) + dz dz) with dx = p_ix - p_jx and so on: fp64 with + - x only, in exactly that association, no contraction and
 *              no fma.  diameter = sqrt(max_{i <= j} d^2), one correctly rounded sqrt at the end -- sqrt is monotone, so this is the toolkit's maximum of
 *              square roots bit for bit.  The pair (i, i) counts: a one-point model has diameter 0.0.  Exact brute force over all pairs: no fp32 filter,
 *              no pruning.
 *   pair       with pair_out, the pair i <= j whose d^2(i, j) equals the maximum with the lowest i, then the lowest j (point indices within the model).
 *              NULL skips the work.
 *   non-finite a model with any NaN or Inf coordinate gets flags bit 0, NaN in all seven outputs and the pair (-1, -1); every other item of the call is
 *              unaffected.  Finite float32 coordinates cannot overflow fp64 here: a finite model always has finite results.  No input makes the call fault.
 * Every value is a minimum or maximum of numbers that do not depend on where they are formed (integer atomics on order-preserving bit patterns): an item's
 * results do not depend on the launch geometry, on the batch or on its place in it.  One launch set a call, whatever n: a box pass, a pass over the tiles
 * (item, i-tile, j-tile at or above it) of all items in one list, and with pair_out a pass that rescans only the tiles whose maximum equals the item's.
 * Host buffers, blocking; runs on the database's stream under its lock; its scratch grows only.  n = 0 returns 0.  SUO_ERR_ARG with a message, nothing launched
 * and no output written: a null database, n < 0, null model_index or info_out with n > 0, a model index outside the database, a model without points.
 * suo_model_info_tiles: the j-tile and i-tile of the tile pass, in points (the sizes at which a model takes another path through it; for tests). */
int suo_model_info(void* mesh_db, int n, const int* model_index,
                   double* info_out /*[n][7]: min_x, min_y, min_z, size_x, size_y, size_z, diameter*/,
                   int* pair_out    /*[n][2] or NULL: the point indices of a diametral pair*/,
                   int* flags_out   /*[n] or NULL: bit 0 = a non-finite coordinate*/);
void suo_model_info_tiles(int* tile, int* itile);

/* ---- bop_toolkit's point-set pose errors: ADD, ADI, PROJ --------------------------------
 * Replaces bop_toolkit_lib/pose_error.py:147-232 (add, adi, proj; misc.py:93-107 project_pts, misc.py:266-276 transform_pts_Rt) over the same mesh database.
 * Every entry is new; nothing above changes.  With E = [R_est|t_est], G = [R_gt|t_gt] and the model's points p_i, i < P:
 *   ADD  = (1 / P) sum_i |E p_i - G p_i|                          (mm)
 *   ADI  = (1 / P) sum_i min_j |G p_i - E p_j|                    (mm)   for every GROUND-TRUTH point the nearest ESTIMATED-pose point: the direction of the
 *                                                                        toolkit's cKDTree(pts_est).query(pts_gt).  suo_pose_errors' float32 ADD-S above is the
 *                                                                        reference meter's and is not this.
 *   PROJ = (1 / P) sum_i |pi(K, E, p_i) - pi(K, G, p_i)|          (px)   pi = (M [p;1])_xy / (M [p;1])_z with M = K [R|t] formed first, divided as given: a
 *                                                                        point behind the camera keeps its finite value, as in the toolkit.
 * All arithmetic is fp64 on the float32 points widened exactly; a transformed coordinate is ((r0 x + r1 y) + r2 z) + t, a squared distance (dx^2 + dy^2) + dz^2,
 * no contraction.  The nearest neighbour is exact (a minimum over all P^2 squared distances, the square root taken once per point).  The sums run in an order
 * that depends on P alone (point i goes to partial sum i % 256; the 256 partial sums are added by a fixed tree): a pair in a batch has the bits it has alone.
 * est == gt gives ADD = ADI = PROJ = 0 exactly.
 * `which` is a bit mask of SUO_POINTS_ADD / _ADI / _PROJ: only ADI costs P^2, and a call that does not ask for it does not pay for it.  An output whose bit
 * is not set is not written and may be NULL; K [n][9] row-major may be NULL without SUO_POINTS_PROJ.
 * One stated deviation, as for suo_pose_errors_bop: a pair with a non-finite transformed point (a NaN or overflowing pose) reports +inf for ADD and ADI, a
 * pair with a non-finite projected distance (z exactly 0) +inf for PROJ.  No input makes the call fault.
 * model_index[n], T_est / T_gt [n][12] row-major 3x4 (doubles, mm).  Host buffers, blocking.  n = 0 or which = 0 return 0.
 * SUO_ERR_ARG (nothing launched): a null database or required pointer, n < 0, an unknown bit in which, a model index outside the database. */
#define SUO_POINTS_ADD 1
#define SUO_POINTS_ADI 2
#define SUO_POINTS_PROJ 4
int suo_pose_errors_points(void* mesh_db, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, int which,
                           double* add_out, double* adi_out, double* proj_out);

/* ---- bop_toolkit's mask pose errors from two renders: CUS, COU_BB_PROJ ------------------
 * What bop_toolkit_lib/pose_error.py:256-286 (cus) and :300-329 (cou_bb_proj) take from the depth images of model_index[i] rendered at T_est[i] and at T_gt[i]
 * under K[i], width x height (the rules of suo_render_depth, unchanged): with mask_est = depth_est > 0 and mask_gt = depth_gt > 0,
 *   counts_out [n][2]   pixels of mask_est | mask_gt (union) and of mask_est & mask_gt (intersection);
 *   box_est, box_gt     [n][4] = [xmin, ymin, xmax - xmin, ymax - ymin] of each mask: no + 1, no clipping (misc.calc_2d_bbox); [-1, -1, -1, -1] for an
 *                       empty mask.
 * The quotients are the caller's, in fp64 from these exact integers:  cus = 1 - intersection / float(union), or 1.0 when union is 0;
 * cou_bb_proj = 1 - misc.iou(box_est, box_gt) (misc.py:236-263).  One stated deviation: the toolkit's cou_bb_proj raises on an empty mask (min() of an empty
 * array); suo_slam_amd.bop_eval reports 1.0 for it, as cus does.
 * Both renders of a pair are drawn tile by tile into two z-buffers in LDS and reduced there; neither depth image is written to memory.  The device writes
 * integers only, reduced per wave, per workgroup and then by one integer atomic per quantity: the values of a pair do not depend on the batch, its order or
 * the tiling.  Every entry is new; nothing above changes.
 * Host buffers, blocking.  n = 0 returns 0.  SUO_ERR_ARG with a message, before anything is launched: as for suo_render_depth (a null pointer, non-finite T
 * or K, a model index out of range, a model without faces, width or height < 1, width * height > 2^28).  More pairs than one launch takes (1024, fewer
 * with many triangles) are split inside. */
int suo_pose_errors_masks(void* mesh_db, int n, const int* model_index, const double* T_est, const double* T_gt, const double* K, int width, int height,
                          long long* counts_out /*[n][2]: union, intersection*/, int* box_est /*[n][4]*/, int* box_gt /*[n][4]*/);

/* ---- SLAM-mode hypothesis scoring------------------------------------------
 * Replaces the per-pair numpy of ObjectSLAM.__estimate_camera_pose's hypothesis loop (lib/object_slam.py:1000-1066) and of
 * __maybe_reinit_objects' inlier counts (:619-690): count_k [ z_k > 0 and chi2_k <= chi2_max ] for n_pairs (pose, detection) pairs in one launch.
 * A detection is written once into a device-resident store (suo_slam_store_put; host rows [n][SUO_SLAM_ROW] doubles:
 *   model keypoints [41][3] | predicted uv [41][2] | covariances [41][2][2] | K_bbox [3][3] row-major | n | has_cov (0 / 1), unused keypoints zero);
 * a pair is SUO_SLAM_PAIR doubles: T [3][4] row-major (detection's object -> camera), the keypoint selection as the 64 bits of a uint64
 * (bit k = keypoint k counts: k < n, and its inlier flag where the reference scores inliers only, :1040), the store slot as the 64 bits of an int64.
 * chi2 = r^T Sigma^-1 r with Sigma's diagonal clamped at 1e-4 (:669,:1054), or |r|^2 / kp_std2 for a detection without covariances.
 * counts_host [n_pairs + 1]: the counts, then a flag: some selected keypoint's chi2 was NaN (the reference asserts on it).  Blocking; host buffers. */
#define SUO_SLAM_ROW 380
#define SUO_SLAM_PAIR 14
void* suo_slam_store_create(int capacity);
void suo_slam_store_destroy(void* store);
int suo_slam_store_put(void* store, int first_slot, int n, const double* rows_host);
int suo_slam_score(void* store, int n_pairs, const double* pairs_host, double chi2_max, double kp_std2, int32_t* counts_host);

/* ---- A view's three-panel visualisation (collect_results(no_viz=False)) ------------------------
 * What lib/object_slam.py:226-274 and lib/utils/utils.py:182-354 (draw_points, bbox_color, make_kp_viz) paint for one view, on the device.  Every entry is
 * new; nothing above changes.  Everything up to the list of primitives is the reference's own arithmetic and is done by the caller
 * (suo_slam_amd/viz.py: build_primitives); how cv2 rasterises a primitive cannot be pinned here (no cv2), so each rule below is stated and marked
 * ORACLE-UNPINNED, as the prior stamp and the VSD rasteriser are.
 *
 * Canvas       frame uint8 [H][W][3] BGR on the device; out uint8 [H][3 W][3]: left | centre | right, each panel starting as a copy of the frame.
 * Colours      a colour is packed b | g << 8 | r << 16.  suo_viz_colours gives the reference's two tables as data: the 41 kp_colors() (kp_config.py:97-102,
 *              the shuffle under seed 123456 included) and the 30 bbox_color() entries (utils.py:248-251).  The caller indexes the second as the reference
 *              does, cols[obj_id - 1] with Python's indexing, and refuses obj_id > 30.
 * Disc         (x, y, r, colour): pixels with dx^2 + dy^2 <= r^2, in integers.                                                          ORACLE-UNPINNED
 * Keypoint     a black disc of radius r_outer = int(round(1.3 rad)), then a disc of radius r_inner = rad in the keypoint's colour, then its ellipse when
 *              has_ellipse (rad = 8 from make_kp_viz).  A keypoint whose rounded centre is off the canvas is not in the list at all (utils.py:216-217):
 *              that is the caller's rule; the device clips whatever it is given.
 * Ellipse      outline (x, y, A, B, cos phi, sin phi, colour), A and B integer half-axes >= 0: with xr = dx cos + dy sin, yr = -dx sin + dy cos in fp64 and
 *              inside(a, b) <=> (xr b)^2 + (yr a)^2 <= (a b)^2, the pixel is painted iff inside(A + 1, B + 1) and not (A >= 2 and B >= 2 and
 *              inside(A - 1, B - 1)).  cos and sin arrive as fp64 from the host; the device uses + - x only, no contraction.               ORACLE-UNPINNED
 * Box          (x1, y1, x2, y2, colour), thickness 3: pixels inside [x1 - 1, x2 + 1] x [y1 - 1, y2 + 1] and not inside [x1 + 2, x2 - 2] x [y1 + 2, y2 - 2],
 *              clipped to the canvas.                                                                                                     ORACLE-UNPINNED
 * Text         putText labels are not drawn (a stated deviation).
 * Order        primitives overwrite in list order, which is the reference's call order: objects in obj_ids order, keypoints in channel order, per keypoint
 *              black disc, colour disc, ellipse.  The last hit wins.
 * Left panel   boxes first.  Then the prior heat: a stamp (channel k, ulx, uly, window x0, x1, y0, y1) contributes float32(w[y - uly] w[x - ulx]) -- the
 *              table of suo_render_priors: w[i] = exp(-(i - 45)^2 / (2 14^2)), doubled at i = 0 -- at pixels with 0 <= x - ulx < 90, 0 <= y - uly < 90 inside
 *              the window x0 <= x < x1, y0 <= y < y1 (the object's box window [y1:y2, x1:x2] exactly as Python's slices select it, formed by the caller with
 *              slice.indices).  Per channel s_k = the float32 sum over the stamps of that channel in list order, clipped to [0, 1];
 *              prior_c = uint8(trunc(clip(sum_k s_k kp_colour[k][c], 0, 255))) summed in fp64 (exact in any order);
 *              g = (1868 b + 9617 g + 4899 r + 8192) >> 14 over prior_c (OpenCV's documented 8-bit BGR2GRAY);                                ORACLE-UNPINNED
 *              in fp32 without contraction p = float(g) / 255, out_c = uint8(trunc((1 - p) img_c + p prior_c)), img being the panel with its boxes.
 *              The [41][H][W] prior tensor never exists in memory.
 * Right panel  overlay objects in paint order (far to near: the caller's stable sort on -T_OtoC[2][3]).  Per float32 mesh point p, widened exactly, in fp64:
 *              X = ((r0 x + r1 y) + r2 z) + t per row, (a, b, c) = K X per row as (k0 X + k1 Y) + k2 Z, u = a / c, v = b / c.  No depth test: the reference
 *              has none.  A point is skipped when u or v is not finite or |u + 0.5| or |v + 0.5| >= 2^31; its pixel is trunc(u + 0.5), trunc(v + 0.5) toward
 *              zero (values in (-1, 0) land on 0, as torch's .to(int) does), kept when inside the canvas.  Each object's mask is dilated by a 3 x 3 square,
 *              nothing entering from outside the canvas, and painted in its colour, later objects over earlier ones.  On the device: an int32 [H][W] owner
 *              plane takes atomicMax(rank + 1) per point, and the painted object of a pixel is the 3 x 3 maximum of that plane -- order-free and exact.
 *              (The reference projects in float32; the rule is fp64, and agrees wherever no projected coordinate sits on a pixel boundary.)
 * One view per call; a batched form is out of scope.  suo_viz_view is stream-ordered and does no host synchronisation: it stages the descriptor in pinned
 * memory, enqueues one copy, the clearing of the owner plane and two kernels on `stream`, and returns.  The pinned staging is a ring of SUO_VIZ_RING slots: the
 * caller must not have more than that many views of one handle in flight, and uses one stream per handle at a time.  frame and out are device pointers, out
 * [H][3 W][3] complete once the stream reaches what is enqueued next; every other array of the descriptor is host memory, free to reuse on return.
 * SUO_ERR_ARG with a message, before anything is launched: a null handle, descriptor, frame or out; a negative count or a null array with a positive count;
 * n_kp > SUO_VIZ_MAX_KP (16 objects x 41 keypoints), n_stamp > SUO_VIZ_MAX_KP, n_box > SUO_VIZ_MAX_OBJ, n_overlay > SUO_VIZ_MAX_OBJ (64); a stamp channel
 * outside [0, 41); a negative radius or half-axis or one above 2^20; a non-finite cos / sin; overlays without a mesh database, or a model index outside it;
 * suo_viz_create: H or W < 1 or H W >= 2^31. */
#define SUO_VIZ_MAX_KP 656
#define SUO_VIZ_MAX_OBJ 64
#define SUO_VIZ_RING 8
typedef struct suo_viz suo_viz;
typedef struct suo_viz_view_desc {
    const uint8_t* frame;            /* device, [H][W][3] BGR */
    int n_box;     const int32_t* box;           /* [n_box][5]: x1, y1, x2, y2, colour */
    int n_stamp;   const int32_t* stamp;         /* [n_stamp][8]: channel, ulx, uly, x0, x1, y0, y1, object (informative) */
    int n_kp;      const int32_t* kp;            /* [n_kp][8]: x, y, r_outer, r_inner, colour, has_ellipse, A, B */
    const double* kp_cs;                         /* [n_kp][2]: cos phi, sin phi (read where has_ellipse) */
    int n_overlay; const int32_t* overlay_model; /* [n_overlay] index into the mesh database, in paint order */
    const int32_t* overlay_colour;               /* [n_overlay] */
    const double* overlay_T;                     /* [n_overlay][12] row-major 3x4 object -> camera */
    const double* overlay_K;                     /* [n_overlay][9] row-major */
} suo_viz_view_desc;
int suo_viz_colours(uint8_t* kp_bgr /*[41][3]*/, uint8_t* box_bgr /*[30][3]*/);
int suo_viz_create(int H, int W, suo_viz** out);
void suo_viz_destroy(suo_viz* viz);
int suo_viz_view(suo_viz* viz, const suo_viz_view_desc* view, void* mesh_db /*suo_mesh_db_create's, may be NULL without overlays*/, uint8_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUO_HIP_H */
