// Host-side runtime object behind suo_net_* (see include/suo_hip.h).
#pragma once
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "suo_internal.h"

namespace suo {

struct HostTensor {
    const float* data = nullptr;
    std::vector<int64_t> shape;
    size_t numel = 0;
};

// one operator's weights in each matrix-pipe form: w[0] fp32 packing, w[1] three bf16 planes, w[2] two fp16 planes; osc: the fp16 form's per-column factors
// (csrc/bf16x3.h, csrc/f16x2.h; a form the operator has no kernel for, or the network was not built for, stays null)
struct PipeW { float* w[3] = {nullptr, nullptr, nullptr}; float* osc = nullptr; };
// w[1]: N a multiple of 128, K segments multiples of 64 (csrc/gemm_bf16x3.hip)
// site / xs16: the fp16 form's activation site of this convolution's input (Net::sites_ index, -1: none) and its factor 2^s in device memory
struct GemmW { PipeW w; float* bias = nullptr; int N = 0, n_valid = 0, K1 = 0, K2 = 0; int site = -1; const float* xs16 = nullptr; };
// Wp: the direct kernels' packing; wino: Winograd-packed (3x3, 128 -> 128 / 64 -> 64; csrc/conv_wino.hip, csrc/conv_wino_x3.hip)
struct ConvW { float* Wp = nullptr; float* bias = nullptr; int N = 0, C = 0, KS = 0; PipeW wino; int site = -1; const float* xs16 = nullptr; };
struct ResidualW {
    float* pro_scale = nullptr; float* pro_shift = nullptr;
    GemmW c1; ConvW c2; GemmW c3;
    int cin = 0, cout = 0; bool has_skip_conv = false;
    PipeW tail;          // conv3 for the fused tail of the 3x3: w[0] is c3.w.w[0] (not a copy); w[1] / w[2] in the Winograd tail's layout (256 <- 128 only)
    // 256 -> 256 blocks: the whole block in one launch on small maps (csrc/res_small.hip fp32 pipe; csrc/res_small_x3.hip bf16 / fp16 pipe)
    PipeW block[3];      // pack_res16_gemm(W1 bn1-folded) | pack_res16_conv3x3(W2, bn2 scale) | pack_res16_gemm(W3), and their planes; factors [128], [128], [256]
};
struct HourglassW {
    int n = 0;
    ResidualW up1[2], low1[2], low2[2], low3[2];
    std::unique_ptr<HourglassW> inner;
};

void pack_gemm_weight(const float* W, int N, int K, int ldw, int Np, int Kp, float* out);
void pack_conv_weight(const float* W, int N, int C, int KS, int Np, int Cp, int CK, const float* out_scale, float* out);

class Net {
public:
    Net(int n, const char* const* names, const float* const* data, const int64_t* const* shapes, const int* ndims, int max_crops);
    ~Net();
    int forward(const void* img, int fmt, int H, int W, const float* boxes, const int* box_img, int L, const float* priors,
                const float* prior_uv, const uint8_t* prior_mask, float* uv, float* cov,
                float* kp_prob, float* kp_logit, float* logits_out, hipStream_t s);
    int forward_staged(const float* in0_user, int L, float* logits_out, hipStream_t s);
    int prepare(int L, int with_priors, hipStream_t s);
    void set_use_graph(bool v) { use_graph_ = v; }
    // matrix pipe of the large launches: 0 = fp32 MFMA, 1 = three bf16 terms (6 MFMAs per product block), 2 = two fp16 terms (3 MFMAs; range-guarded)
    int pipe() const { return pipe_; }
    int set_pipe(int p);
    // 1 when a forward since the last call of this function left the fp16 range (its outputs are invalid); clears the flag.  The caller has synchronised.
    int range_exceeded();
    // per-call validity: the number of the last forward issued (1, 2, ...), and whether THAT call left the fp16 range (1), did not (0), or cannot be answered (-1:
    // not finished, or older than the last kCallRing calls).  On 1 the network has moved to the bf16 form.  The caller has synchronised on the call's outputs.
    uint64_t last_call() const { return calls_; }
    int call_range_exceeded(uint64_t call);
    int max_crops() const { return max_crops_; }
    // per-site activation exponents of the fp16 form (csrc/f16x2.h): sites in a fixed order, named by their convolution's state-dict prefix
    int f16x2_sites() const { return (int)sites_.size(); }
    const char* f16x2_site_name(int i) const { return i >= 0 && i < (int)sites_.size() ? sites_[i].name.c_str() : nullptr; }
    int get_f16x2_shifts(int* out, int n) const;
    int set_f16x2_shifts(const int* s, int n);
    // one probe forward of the prior-less pass on the bf16x3 form, max |operand| per site, s by the rule; not a numbered call, the range record untouched
    int calibrate(const void* img, int fmt, int H, int W, const float* boxes, const int* box_img, int L, hipStream_t s);
    size_t workspace_bytes() const { return ws_floats_ * sizeof(float); }
    int schedule_bytes(int L, int n_frames, int H, int W, int with_priors, double* out, int* n_launches);
    const HostTensor& T(const std::string& name) const;

private:
    static constexpr int kNumSide = 4, kNumEvents = 32;
    // the range guard's words in mapped host memory (range_flag_): [kLiveWord] raised by the fp16 kernels of the call that is running; [kStickyWord] set when a
    // committed call had raised it, cleared by range_exceeded(); [kSlotWord + i] the result of call c with c % kCallRing == i, as (c mod 2^31) * 2 + raised
    static constexpr int kCallRing = 64, kLiveWord = 0, kStickyWord = 16, kSlotWord = 32;
    int commit_call(hipStream_t s);
    void leave_fp16_form();
    bool own_call_invalid();
    // ---- weights (csrc/net_weights.hip)
    void build_weights(int n, const char* const* names, const float* const* data, const int64_t* const* shapes, const int* ndims);
    float* upload(const std::vector<float>& v);
    template <class Pack3, class Pack2>
    void fill_pipes(PipeW& pw, const float* src, size_t numel, int ncol, Pack3 pack3, Pack2 pack2, bool with_bf16 = true);
    void make_gemm(const std::string& conv, const std::string& bn_after, const std::string& conv2, GemmW& g);
    void pack_gemm(const std::vector<float>& full, const std::vector<float>& bias, int N, int K1, int K2, GemmW& g);
    void make_conv(const std::string& conv, const std::string& bn_after, int CK, ConvW& c, int c_used = 0);
    void make_residual(const std::string& p, ResidualW& r);
    void make_hourglass(const std::string& p, int n, HourglassW& h);
    float* alloc(size_t floats);
    // How one Residual block runs at one call shape: the route (which launches), the form each launch runs on (0 = fp32 MFMA, 1 = three bf16 terms, 2 = two
    // fp16 terms) and what the route can do for its neighbours.  Net::plan_block is the only place that decides any of it; residual() and hourglass() read it.
    struct BlockPlan {
        enum Route { ONE_LAUNCH,       // the whole block in one launch (csrc/res_small.hip: form 0; csrc/res_small_x3.hip: forms 1 and 2)
                     DIRECT_FUSED,     // conv1 | direct 3x3 + conv3 + skip (csrc/conv.hip: FUSE)
                     WINO_FUSED,       // conv1 | Winograd 3x3 + conv3 + skip [+ up-sampled addend] [+ the next block's conv1]
                     PER_LAYER };      // conv1 | 3x3 | conv3 (+ conv4)
        Route route = PER_LAYER;
        bool wino = false;                     // the 3x3 on the Winograd kernels (else the direct kernel, fp32 pipe)
        int form = 0;                          // of the one-launch block / the Winograd 3x3 and its tail
        int form1 = 0, form3 = 0;              // of conv1 / conv3 as launches of their own (gemm_form)
        bool takes_up = false;                 // the route adds an up-sampled addend itself (residual() refuses `up` on any other before it enqueues anything)
        bool can_carry_next_conv1 = false;     // its tail can also compute the conv1 of the block that follows at this resolution (without `up` / `pool_out`)
        bool uses_producer_conv1 = false;      // as a consumer: the route takes a conv1 its producer computed (pre_) -- a fused fp16 tail's, or the fused stem's for r1
    };
    BlockPlan plan_block(const ResidualW& r, int L, int H, int W) const;
    // pool_out: also produce max_pool2d(out, 2, 2) (fused into the last GEMM where it can be, else a separate launch); `out` may then be nullptr
    // next: the Residual block that consumes `out` next at this resolution (or nullptr): where this block's plan can carry next's conv1 and next's plan uses
    // it, the tail launch also computes it (csrc/conv_wino_x3.hip, NEXT) and residual(*next, out, ...) finds it done (pre_*)
    int residual(const ResidualW& r, const float* x, float* out, int L, int H, int W, hipStream_t s, const float* up = nullptr, float* pool_out = nullptr,
                 const ResidualW* next = nullptr);
    long wino_min_tiles() const;
    long x3_min_rows() const;
    int gemm_form(const GemmW& gw, long M) const;
    int gemm_maybe_pooled(GemmArgs& g, int L, int H, int W, float* pool_out, hipStream_t s, const GemmW& gw, int form);
    int residual_one_launch(const ResidualW& r, const BlockPlan& p, const float* x, float* out, int L, int H, int W, hipStream_t s, const float* up, bool pool_in);
    std::pair<float*, float*> layout_slabs();      // {staged input, logits}
    int hourglass(const HourglassW& h, const float* x, float* out, int L, int H, int W, hipStream_t s, int depth_idx, const float* x_pooled = nullptr);
    int backbone(const float* in0, int in_c, float* logits, int L, hipStream_t s, bool stem_done = false);
    int run_backbone(float* in0, int in_c, float* logits, int L, hipStream_t s, bool stem_done = false);
    int ensure_graph(float* in0, int in_c, float* logits, int L, hipStream_t s, hipGraphExec_t* exec, bool stem_done = false);
    bool fused_stem() const;
    int follow_null_stream();

    // ---- fp16 activation sites
    static constexpr int kMaxSites = 256;
    struct Site {
        std::string name; int ksize = 1; int shift = 4;
        std::vector<std::pair<float*, std::vector<float>>> osc;       // the device factor arrays of the site's convolution and their values at s = S2_XSHIFT
    };
    std::vector<Site> sites_;
    float* site_xs_ = nullptr;                           // [kMaxSites] device: 2^s per site (the kernels read it through GemmW / ConvW::xs16)
    unsigned* probe_max_ = nullptr;                      // [kMaxSites] device: the probe's max |operand| per site (float bits)
    bool probe_ = false;                                 // the schedule of the calibration probe: per-layer launches on the bf16x3 / fp32 forms, every operand materialised
    std::vector<char> probed_;                           // ... which sites it measured
    int add_site(const std::string& name, int ksize);
    void site_osc(int site, float* dev, int n);
    void register_residual_sites(const std::string& p, ResidualW& r);
    void register_gemm_site(const std::string& p, GemmW& g);
    int apply_shifts(const std::vector<int>& s);
    int probe_site(int site, const float* x, long rows, int C, int ld, const float* scale, const float* shift, int relu, hipStream_t s);

    std::map<std::string, HostTensor> tensors_;
    std::vector<float*> owned_;
    ConvW stem_, stem_img_;      // all 44 input channels | the 3 image channels only (no priors: SLAM_C = 16)
    PipeW stem_x3_; float* stem_x3_bias_ = nullptr;                   // the image-only stem for the fused RoIAlign + stem launch (csrc/stem_x3.hip; no fp32 form: w[0] null)
    float* stem_slab_ = nullptr;                                      // [max_crops,128,128,64] persistent slab of the stem's output
    float* stem_mid1_slab_ = nullptr;                                 // ... and of r1's conv1 when the fused stem launch computes it (csrc/stem_x3.hip: NEXT)
    bool stem_computes_r1_conv1() const;
    ResidualW r1_, r4_, r5_, post_[2][2];
    HourglassW hg_[2];
    GemmW lin_[2], head_[2], reinject_;
    float* cls_w_ = nullptr; float* cls_b_ = nullptr;
    int max_crops_;
    float* ws_ = nullptr; size_t ws_floats_ = 0, ws_used_ = 0, ws_mark_ = 0;
    float* d_mean_logit_ = nullptr;
    hipStream_t side_[kNumSide] = {}; hipStream_t own_stream_ = nullptr;
    hipEvent_t ev_[kNumEvents] = {}; int ev_next_ = 0;
    bool use_graph_ = true; bool dry_run_ = false;
    bool acct_on_ = false; double acct_[8] = {}; int acct_launches_ = 0;      // schedule_bytes: algorithmic HBM bytes per kind of launch, summed over a dry run
    void acct(int kind, double bytes) { if (acct_on_) acct_[kind] += bytes; }
    int maxpool(const float* in, float* out, int L, int H, int W, int C, hipStream_t s);
    struct PreConv1 { const float* x; const ResidualW* r; float* mid1; };      // conv1 of block r on input x, already computed by the producer's tail
    std::vector<PreConv1> pre_;                                              // (several can be pending: up1[0]'s for up1[1] waits while the low branch runs)
    int pipe_ = 1, pipe_built_ = 1;                      // the pipe in use / the best one the weights were packed for
    unsigned* range_flag_ = nullptr;                     // mapped host memory: the f16x2 kernels raise it, the host reads it after any synchronisation
    uint64_t calls_ = 0;                                 // forwards issued (commit_call numbers them)
    int call_pipe_[kCallRing] = {};                      // ... and the pipe each of the last kCallRing ran on
    // two executables per captured graph, launched alternately: hipGraphLaunch of an executable whose previous launch is still running blocks the host until
    // that one ends (measured: 14 ms per call with a second batch in flight behind ObjectSLAM.submit_views_single) -- with two, the host runs ahead by one call
    struct GraphEntry { hipGraph_t graph = nullptr; hipGraphExec_t exec[2] = {nullptr, nullptr}; int next = 0; };
    std::map<int, GraphEntry> graphs_;
};

}  // namespace suo
