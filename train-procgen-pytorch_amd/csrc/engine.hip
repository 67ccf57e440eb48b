// Context, network program and the C ABI (include/mi355ppo.h) of the MI355X PPO hot path.
//
// Device-resident state per context (one per GPU):
//   rollout ring   frames uint8 NHWC [(T+1)][E][64][64][3]  (or fp32 [(T+1)][E][obs_dim] for the MLP)
//                  rew/done/logp/adv/ret fp32 [T][E], act int32 [T][E], value fp32 [T+1][E]
//   parameters     ONE flat fp32 buffer (+ grad, exp_avg, exp_avg_sq of the same shape): filter banks
//                  as [co][tap][ci], fc columns in NHWC-flatten order, heads as one (A+1) x H matrix
//   activations    NHWC fp32, every tensor the backward pass needs, sized for max_batch samples
// The reference keeps all of this on the host in fp32 and re-uploads a gathered minibatch for every
// update (common/storage.py:112-128); here the minibatch gather is an index read inside the first conv.
//
// File map:
//   engine_ctx.h    mi_ctx and the structs it embeds, the error plumbing (fail, HIPC, ARG, NETCHK, JOIN, CUR), and the declarations of
//                   the functions of this file and of rollout.hip that another file calls
//   lanes.h         which stream an env group of the pipelined rollout runs on: the process-wide lane registry (plain C++, host-tested)
//   group_worker.h  how a step reaches an env group's worker thread and its result comes back: the hand-off (plain C++, host-tested)
//   devpool.h       who frees what: the pool that owns a context's device buffers, pinned buffers and events (plain C++, host-tested)
//   engine.hip      create / destroy, layout tables, parameter and field I/O, profiler, the network program (forward_* / backward_* per
//                   mode), estimates, minibatch passes, optimizer, GRU training, collectives
//   rollout.hip     rollout steps, env groups (lanes, workers, submit / wait, teardown), the staged entries (predict, saliency, commit,
//                   forward) and the recurrent rollout's state: host code only, no kernel
//   engine_ops.hip  mi_op_*, mi_debug_* (but mi_debug_flags: it sets production state) and mi_selftest_mfma: tests and micro-benchmarks only
//
// A minibatch pass in launch order (bf16 IMPALA at update size; minibatch_impl -> net_forward -> loss -> net_backward):
//    1 stage_indices           pull the minibatch indices into d_idx
//    2 forward_impala_bf16     repack (after an optimizer step), conv1+pool, per block: conv+pool, residual pair; fc
//    3 net_heads               logits + value
//    4 loss                    loss_fwd_seg (+ fs_metric_seg, loss_finalize_seg here when the pass has no side job)
//    5 heads_backward          dY -> dfeat, head gradients                          | fork 1 (fork_stats_and_fc): head slab sum, metric,
//    6 fc data gradient        dfeat -> block-3 output gradient                     |   log records, fc weight / bias gradients
//    7 blocks 3, 2, 1          backward_residual_pair, then the block's conv (+ pool) backward
//    8 block1.conv wgrad       last kernel of the pass                              | fork 2 (fork_slab_sums): the first 14 slab sums
//    9 join, slab sum          the remaining slab sum(s) into the flat gradient
//   10 mi_optimizer_step       gradient norm + Adam (its own entry point)
#include "engine_ctx.h"

thread_local std::string g_err;
__thread hipStream_t tl_stream = nullptr;
__thread float* tl_ws = nullptr;
__thread size_t tl_ws_floats = 0;
const char* mi_last_error(void) { return g_err.c_str(); }

// ---- the HIP backend of every pool (devpool.h), and the process-wide counts of what the pools hold: device allocations, pinned
// allocations, events (mi_debug_live_resources: back at their earlier values once a context is destroyed)
static std::atomic<int64_t> g_live[3];
static int hip_dev_alloc(void** p, size_t bytes, bool zero) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return e;
    // hipMemset is asynchronous on the NULL stream and the context's stream is non-blocking: without this wait a
    // kernel launched right after (the op-level test hooks do that) can be overtaken by the zero fill
    if (zero && ((e = hipMemset(*p, 0, bytes)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)) { hipFree(*p); return e; }
    ++g_live[0];
    return 0;
}
static void hip_dev_free(void* p) { hipFree(p); --g_live[0]; }
static int hip_pinned_alloc(void** p, size_t bytes, unsigned flags) { const hipError_t e = hipHostMalloc(p, bytes, flags); g_live[1] += e == hipSuccess; return e; }
static void hip_pinned_free(void* p) { hipHostFree(p); --g_live[1]; }
static int hip_event_create(void** ev, unsigned flags) { const hipError_t e = hipEventCreateWithFlags((hipEvent_t*)ev, flags); g_live[2] += e == hipSuccess; return e; }
static void hip_event_destroy(void* ev) { hipEventDestroy((hipEvent_t)ev); --g_live[2]; }
const DevPool::Backend* hip_pool() {
    static const DevPool::Backend be = {hip_dev_alloc, hip_dev_free, hip_pinned_alloc, hip_pinned_free, hip_event_create, hip_event_destroy};
    return &be;
}
int mi_debug_live_resources(int64_t out[3]) { ARG(out, "null"); for (int k = 0; k < 3; ++k) out[k] = g_live[k].load(); return 0; }

#define NCCLC(x)                                                                                         \
    do {                                                                                                 \
        ncclResult_t r_ = (x);                                                                           \
        if (r_ != ncclSuccess) return fail(-5, std::string(#x) + ": " + ncclGetErrorString(r_) + " @" + std::to_string(__LINE__)); \
    } while (0)

extern "C" int mi_comm_destroy(mi_ctx* c);
static void prof_harvest(mi_ctx* c);
static const char* kProfNames[PC_COUNT] = {
    "conv_fwd_3_16_64", "conv_fwd_16_16_32", "conv_fwd_16_32_32", "conv_fwd_32_32_16", "conv_fwd_32_32_8",
    "conv_dgrad_3_16_64(unused)", "conv_dgrad_16_16_32", "conv_dgrad_16_32_32", "conv_dgrad_32_32_16", "conv_dgrad_32_32_8",
    "conv_wgrad_3_16_64", "conv_wgrad_16_16_32", "conv_wgrad_16_32_32", "conv_wgrad_32_32_16", "conv_wgrad_32_32_8",
    "maxpool_fwd", "maxpool_bwd", "gemm", "slab_reduce",
    "resblock_fwd_(unused)", "resblock_fwd_16_16_32", "resblock_fwd_(unused)", "resblock_fwd_32_32_16", "resblock_fwd_32_32_8",
    "resblock_dgrad_(unused)", "resblock_dgrad_16_16_32", "resblock_dgrad_(unused)", "resblock_dgrad_32_32_16", "resblock_dgrad_32_32_8"};

// the few lines every entry point used to spell out by hand
struct GemmWs { float* p; size_t floats; };
static inline GemmWs gemm_ws(mi_ctx* c) { return tl_ws ? GemmWs{tl_ws, tl_ws_floats} : GemmWs{c->gemm_ws, c->gemm_ws_floats}; }   // split-K workspace (a group worker: its slice)
// the first env group's lane when there is one (idle during an update, joined by JOIN(); one hardware queue less in use), else an own stream
static hipStream_t side_stream(mi_ctx* c) {
    hipStream_t ss = (c->n_groups > 0 && c->grp[0].stream) ? c->grp[0].stream : c->side_stream;
    if (!ss) { hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking); ss = c->side_stream; }
    return ss;
}
static int64_t gru_count(const mi_ctx* c) { return 2 * (int64_t)3 * c->H * c->H + 2 * (int64_t)3 * c->H; }      // floats of the four GRU tensors

// ------------------------------------------------------------------------------------------ layout tables
static void add_tensor(mi_ctx* c, const std::string& name, int64_t n, int kind, int co, int ci, int64_t& ref, int64_t dev) {
    TensorDesc t{name, ref, dev, n, kind, co, ci};
    c->tensors.push_back(t);
    ref += n;
}

std::string net_err_take(mi_ctx* c) { std::lock_guard<std::mutex> lk(c->net_err_mu); std::string m; m.swap(c->net_err); return m; }
void net_err_set(mi_ctx* c, const std::string& m) { std::lock_guard<std::mutex> lk(c->net_err_mu); if (c->net_err.empty()) c->net_err = m; }

static void build_impala_layout(mi_ctx* c) {
    // reference order = policy.parameters(): embedder.block{1,2,3}.{conv,res1.conv1,res1.conv2,res2.conv1,res2.conv2}.{weight,bias},
    // embedder.fc.{weight,bias}, fc_policy.{weight,bias}, fc_value.{weight,bias}   
    const int chan[4] = {3, 16, 32, 32};
    const ConvShape first[3] = {CS_3_16_64, CS_16_32_32, CS_32_32_16};
    const ConvShape resid[3] = {CS_16_16_32, CS_32_32_16, CS_32_32_8};
    const char* sub[5] = {"conv", "res1.conv1", "res1.conv2", "res2.conv1", "res2.conv2"};
    int64_t ref = 0;
    for (int b = 0; b < 3; ++b)
        for (int k = 0; k < 5; ++k) {
            const int ci = (k == 0) ? chan[b] : chan[b + 1], co = chan[b + 1];
            const std::string base = "embedder.block" + std::to_string(b + 1) + "." + sub[k];
            ConvLayer L;
            L.shape = (k == 0) ? first[b] : resid[b];
            conv_shape_dims(L.shape, &L.cin, &L.cout, &L.hw);
            L.w_off = ref;
            add_tensor(c, base + ".weight", (int64_t)co * ci * 9, K_CONVW, co, ci, ref, ref);
            L.b_off = ref;
            add_tensor(c, base + ".bias", co, K_PLAIN, 0, 0, ref, ref);
            c->convs.push_back(L);
        }
    c->fc.in = 2048; c->fc.out = c->H;
    c->fc.w_off = ref; add_tensor(c, "embedder.fc.weight", (int64_t)c->H * 2048, K_FCW, c->H, 2048, ref, ref);
    c->fc.b_off = ref; add_tensor(c, "embedder.fc.bias", c->H, K_PLAIN, 0, 0, ref, ref);
    const int64_t h0 = ref;
    c->wh_off = h0; c->bh_off = h0 + (int64_t)(c->A + 1) * c->H;
    add_tensor(c, "fc_policy.weight", (int64_t)c->A * c->H, K_PLAIN, 0, 0, ref, c->wh_off);
    add_tensor(c, "fc_policy.bias", c->A, K_PLAIN, 0, 0, ref, c->bh_off);
    add_tensor(c, "fc_value.weight", c->H, K_PLAIN, 0, 0, ref, c->wh_off + (int64_t)c->A * c->H);
    add_tensor(c, "fc_value.bias", 1, K_PLAIN, 0, 0, ref, c->bh_off + c->A);
    c->n_params = ref;
}
// The armed gradient exchange splits the flat gradient at embedder.fc.weight: region B = [0, fc.w_off) must hold exactly the conv
// layers, region A = [fc.w_off, n_params) the fc layer and the heads (net_backward).  Checked once per context.
static bool impala_regions_ok(const mi_ctx* c) {
    for (const ConvLayer& L : c->convs)
        if (L.w_off < 0 || L.b_off <= L.w_off || L.b_off + L.cout > c->fc.w_off) return false;
    return c->fc.w_off < c->fc.b_off && c->fc.b_off + c->H <= c->wh_off && c->wh_off < c->bh_off && c->bh_off + c->A + 1 == c->n_params;
}

static void build_mlp_layout(mi_ctx* c) {
    // MLPModel (common/model.py:954-980): Linear(in,w) ReLU [Linear(w,w) ReLU]*(depth-2) Linear(w,latent)
    const int d = c->cfg.mlp_depth, w = c->cfg.mlp_width;
    int64_t ref = 0;
    auto lin = [&](const std::string& nm, int in, int out) {
        Linear L; L.in = in; L.out = out;
        L.w_off = ref; add_tensor(c, nm + ".weight", (int64_t)in * out, K_PLAIN, 0, 0, ref, ref);
        L.b_off = ref; add_tensor(c, nm + ".bias", out, K_PLAIN, 0, 0, ref, ref);
        c->mlp.push_back(L);
    };
    lin("embedder.model.0", c->cfg.obs_dim, w);
    for (int k = 0; k < d - 2; ++k) lin("embedder.model.2." + std::to_string(2 * k), w, w);
    lin("embedder.model.3", w, c->H);
    const int64_t h0 = ref;
    c->wh_off = h0; c->bh_off = h0 + (int64_t)(c->A + 1) * c->H;
    add_tensor(c, "fc_policy.weight", (int64_t)c->A * c->H, K_PLAIN, 0, 0, ref, c->wh_off);
    add_tensor(c, "fc_policy.bias", c->A, K_PLAIN, 0, 0, ref, c->bh_off);
    add_tensor(c, "fc_value.weight", c->H, K_PLAIN, 0, 0, ref, c->wh_off + (int64_t)c->A * c->H);
    add_tensor(c, "fc_value.bias", 1, K_PLAIN, 0, 0, ref, c->bh_off + c->A);
    c->n_params = ref;
}

// reference layout <-> device layout for one tensor (host side)
void to_device_layout(const TensorDesc& t, const float* ref, float* dev) {
    if (t.kind == K_CONVW) {            // [co][ci][3][3] -> [co][tap][ci]
        for (int co = 0; co < t.co; ++co)
            for (int ci = 0; ci < t.ci; ++ci)
                for (int tap = 0; tap < 9; ++tap) dev[((int64_t)co * 9 + tap) * t.ci + ci] = ref[((int64_t)co * t.ci + ci) * 9 + tap];
    } else if (t.kind == K_FCW) {       // columns c*64 + h*8 + w (NCHW flatten, model.py:54-56) -> (h*8+w)*32 + c
        for (int o = 0; o < t.co; ++o)
            for (int ch = 0; ch < 32; ++ch)
                for (int p = 0; p < 64; ++p) dev[(int64_t)o * 2048 + p * 32 + ch] = ref[(int64_t)o * 2048 + ch * 64 + p];
    } else memcpy(dev, ref, t.n * sizeof(float));
}
void to_ref_layout(const TensorDesc& t, const float* dev, float* ref) {
    if (t.kind == K_CONVW) {
        for (int co = 0; co < t.co; ++co)
            for (int ci = 0; ci < t.ci; ++ci)
                for (int tap = 0; tap < 9; ++tap) ref[((int64_t)co * t.ci + ci) * 9 + tap] = dev[((int64_t)co * 9 + tap) * t.ci + ci];
    } else if (t.kind == K_FCW) {
        for (int o = 0; o < t.co; ++o)
            for (int ch = 0; ch < 32; ++ch)
                for (int p = 0; p < 64; ++p) ref[(int64_t)o * 2048 + ch * 64 + p] = dev[(int64_t)o * 2048 + p * 32 + ch];
    } else memcpy(ref, dev, t.n * sizeof(float));
}

static int upload_flat(mi_ctx* c, float* dbuf, const float* flat, int64_t n) {
    ARG(n == c->n_params, "flat vector length != mi_param_count"); JOIN(c);
    std::vector<float> tmp(n);
    for (auto& t : c->tensors) to_device_layout(t, flat + t.ref_off, tmp.data() + t.dev_off);
    HIPC(hipMemcpyAsync(dbuf, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
static int download_flat(mi_ctx* c, const float* dbuf, float* flat, int64_t n) {
    ARG(n == c->n_params, "flat vector length != mi_param_count"); JOIN(c);
    std::vector<float> tmp(n);
    HIPC(hipMemcpyAsync(tmp.data(), dbuf, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    for (auto& t : c->tensors) to_ref_layout(t, tmp.data() + t.dev_off, flat + t.ref_off);
    return 0;
}

// ------------------------------------------------------------------------------------------ create / destroy
static int ctx_build(mi_ctx* c);
static void ctx_release(mi_ctx* c);
int mi_create(const mi_config* cfg, mi_ctx** out) {
    ARG(cfg && out, "null cfg/out");
    ARG(cfg->arch == MI_ARCH_IMPALA || cfg->arch == MI_ARCH_MLP, "arch");
    ARG(cfg->n_actions >= 1 && cfg->n_actions <= 16, "n_actions must be in [1,16]");
    ARG(cfg->n_steps >= 1 && cfg->n_envs >= 1 && cfg->max_batch >= 1, "n_steps/n_envs/max_batch");
    ARG(cfg->precision == 0 || cfg->precision == 1, "precision must be 0 (fp32) or 1 (bf16 activations)");
    ARG(cfg->value_from_logits == 0 || cfg->value_from_logits == 1, "value_from_logits must be 0 (fc_value head) or 1 (logsumexp of the logits)");
    if (cfg->arch == MI_ARCH_MLP) ARG(cfg->obs_dim >= 1 && cfg->mlp_depth >= 2 && cfg->mlp_width >= 1 && cfg->out_dim >= 1, "mlp dims");
    // every linear layer's bias gradient is a column sum over its output width (linear_wgrad -> launch_colsum_acc, COLSUM_MAX_N columns)
    if (cfg->arch == MI_ARCH_MLP) ARG(cfg->mlp_width <= COLSUM_MAX_N && cfg->out_dim <= COLSUM_MAX_N, "mlp_width and the MLP's out_dim must be at most 4096 (the bias gradients' column-sum workspace)");
    if (cfg->arch == MI_ARCH_IMPALA)         // out_dim 0: unset by a C caller, the reference's default 256
        ARG(cfg->out_dim == 0 || (cfg->out_dim >= 64 && cfg->out_dim <= 512 && cfg->out_dim % 64 == 0),
            "impala out_dim (output_dim) must be a multiple of 64 in [64, 512]");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(-3, "no HIP device: the MI355X library has no CPU fallback");
    ARG(cfg->device >= 0 && cfg->device < ndev && cfg->device < MAX_LANE_DEVICES, "device");
    HIPC(hipSetDevice(cfg->device));
    mi_ctx* c = new mi_ctx();
    c->cfg = *cfg;
    if (int r = ctx_build(c)) { const std::string why = g_err; ctx_release(c); return fail(r, why); }      // whatever it got so far goes back
    *out = c;
    return 0;
}
// Everything the context owns from its first call on (c->cfg is set, every other member has its default).  It may fail anywhere:
// what it acquired is in the pool or is one of the explicit streams, and ctx_release takes a half-built context.
static int ctx_build(mi_ctx* c) {
    const mi_config* cfg = &c->cfg;
    DevPool& m = c->pool;
    c->T = cfg->n_steps; c->E = cfg->n_envs; c->A = cfg->n_actions;
    c->H = (cfg->arch == MI_ARCH_IMPALA && cfg->out_dim == 0) ? 256 : cfg->out_dim;
    c->NB = cfg->max_batch < cfg->n_envs ? cfg->n_envs : cfg->max_batch;
    c->bf = (cfg->arch == MI_ARCH_IMPALA) && cfg->precision == 1;
    c->lse = cfg->value_from_logits;
    c->es = c->bf ? 2.0 : 4.0;
    if (cfg->stream) c->stream = (hipStream_t)cfg->stream;
    else { HIPC(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    c->main_stream = c->stream;
    HIPC(m.event(&c->ev_side_fork, hipEventDisableTiming)); HIPC(m.event(&c->ev_side_join, hipEventDisableTiming));
    if (cfg->arch == MI_ARCH_IMPALA) build_impala_layout(c); else build_mlp_layout(c);
    if (cfg->arch == MI_ARCH_IMPALA && !impala_regions_ok(c)) return fail(-1, "internal: parameter layout does not split at embedder.fc.weight");

    const int64_t P = c->n_params, T = c->T, E = c->E, NB = c->NB;
    HIPC(m.dev(&c->params, P)); HIPC(m.dev(&c->grads, P)); HIPC(m.dev(&c->adam_m, P)); HIPC(m.dev(&c->adam_v, P));
    HIPC(m.dev(&c->rew, T * E)); HIPC(m.dev(&c->done, T * E)); HIPC(m.dev(&c->logp, T * E));
    HIPC(m.dev(&c->adv, T * E)); HIPC(m.dev(&c->ret, T * E)); HIPC(m.dev(&c->value, (T + 1) * E));
    HIPC(m.dev(&c->act, T * E)); HIPC(m.dev(&c->adv_stats, 4));
    if (cfg->arch == MI_ARCH_IMPALA) {
        c->obs_bytes_per_env = 64 * 64 * 3;
        HIPC(m.dev(&c->frames, (size_t)(T + 1) * E * c->obs_bytes_per_env));
        HIPC(m.dev(&c->stage_frames, (size_t)NB * c->obs_bytes_per_env));
        const int chan[4] = {3, 16, 32, 32};
        int hin = 64;
        for (int b = 0; b < 3; ++b) {
            Block& k = c->blk[b];
            k.cin = chan[b]; k.cout = chan[b + 1]; k.hin = hin;
            const size_t X = (size_t)NB * hin * hin * k.cout, p = X / 4;
            if (!c->bf) HIPC(m.dev(&k.C, X));   // conv output before the pool: bf16 mode keeps it in LDS (fused conv + pool kernels)
            HIPC(m.dev(&k.PI, p));
            HIPC(m.dev(&k.P0, p)); HIPC(m.dev(&k.A1, p)); HIPC(m.dev(&k.P1, p)); HIPC(m.dev(&k.A2, p)); HIPC(m.dev(&k.P2, p));
            hin /= 2;
        }
        if (!c->bf) HIPC(m.dev(&c->GC, (size_t)NB * 64 * 64 * 16));      // gradient of the pre-pool conv output: bf16 mode rebuilds it in LDS (PoolStage)
        for (int k = 0; k < 3; ++k) HIPC(m.dev(&c->GP[k], (size_t)NB * 32 * 32 * 16));
        // every conv layer owns a slab region (persistent grids never exceed 4 workgroups x 256 CUs)
        for (size_t l = 0; l < c->convs.size() && l < 15; ++l) {
            c->slab_off[l] = (long long)c->slab_floats;
            c->slab_floats += (size_t)1024 * (size_t)(c->convs[l].cout * 9 * c->convs[l].cin + c->convs[l].cout);
        }
        HIPC(m.dev(&c->slabs, c->slab_floats));
        HIPC(m.dev_raw(&c->d_slab_desc, sizeof(SlabDesc) * 15));
        HIPC(m.dev(&c->fs_scratch, (size_t)MI_MAX_SEG * 128 * 2048));      // (segments x) FS_GROUPS x 2048 partial column maxima (loss.hip)
        HIPC(m.dev(&c->fs_colmax, (size_t)2048)); HIPC(m.dev(&c->fs_arg, (size_t)2048));
        HIPC(m.dev(&c->fs_keys, (size_t)2048)); HIPC(m.dev(&c->fs_keys_local, (size_t)2048)); HIPC(m.dev(&c->d_gpos, (size_t)NB));
        HIPC(m.pinned(&c->h_gpos, (size_t)NB * 4, hipHostMallocDefault));
    } else {
        c->obs_bytes_per_env = (size_t)cfg->obs_dim * sizeof(float);
        HIPC(m.dev(&c->obsf, (size_t)(T + 1) * E * cfg->obs_dim));
        HIPC(m.dev(&c->stage_obs, (size_t)NB * cfg->obs_dim));
        c->mlp_act.resize(c->mlp.size() + 1);
        HIPC(m.dev(&c->mlp_act[0], (size_t)NB * cfg->obs_dim));
        for (size_t l = 0; l < c->mlp.size(); ++l) HIPC(m.dev(&c->mlp_act[l + 1], (size_t)NB * c->mlp[l].out));
        const int wmax = cfg->mlp_width > c->H ? cfg->mlp_width : c->H;
        for (int k = 0; k < 2; ++k) HIPC(m.dev(&c->GP[k], (size_t)NB * wmax));
    }
    HIPC(m.dev(&c->feat, (size_t)NB * c->H)); HIPC(m.dev(&c->dfeat, (size_t)NB * c->H));
    HIPC(m.dev(&c->hout, (size_t)NB * (c->A + 1))); HIPC(m.dev(&c->dY, (size_t)NB * (c->A + 1)));
    if (c->lse) HIPC(m.dev(&c->d_val, (size_t)NB));
    HIPC(m.dev(&c->d_lp, (size_t)NB * c->A));
    const size_t gws = (size_t)8 << 20;
    HIPC(m.dev(&c->gemm_ws, gws)); c->gemm_ws_floats = gws;
    HIPC(m.dev(&c->col_ws, (size_t)64 * COLSUM_MAX_N));
    HIPC(m.dev(&c->fs_val, 4));
    {
        float h[256];
        for (int k = 0; k < 256; ++k) h[k] = (float)((double)k / 255.0);   // ScaledFloatFrame: obs / 255.0 in fp64, then fp32
        HIPC(m.dev(&c->lut, 256));
        HIPC(hipMemcpy(c->lut, h, sizeof(h), hipMemcpyHostToDevice));
        std::vector<uint16_t> b = host_to_bf16(h, 256);      // the same table as bf16
        HIPC(m.dev(&c->lut16, 256));
        HIPC(hipMemcpy(c->lut16, b.data(), 512, hipMemcpyHostToDevice));
    }
    HIPC(m.dev(&c->d_idx, (size_t)NB));
    HIPC(m.dev(&c->loss_partial, (size_t)(loss_blocks(NB) + 1 + MI_MAX_SEG) * 32));
    HIPC(m.dev(&c->loss_stats, 64));
    HIPC(m.dev(&c->loss_log, (size_t)c->log_cap * 8));
    HIPC(m.dev(&c->stats_ring, (size_t)c->log_cap * 32)); HIPC(m.dev(&c->fs_ring, (size_t)c->log_cap)); HIPC(m.dev(&c->fs_parts, (size_t)MI_MAX_SEG * 8));
    HIPC(m.dev(&c->sumsq, 2 + 128)); HIPC(m.dev(&c->gnorm, 2));
    HIPC(m.dev(&c->d_u, (size_t)E));
    HIPC(m.dev(&c->d_pack, (size_t)3 * E)); HIPC(m.dev(&c->d_rd, (size_t)2 * E));
    // written / read by a RUNNING kernel while the host polls the ticket: fine-grained coherent mapping, whatever HIP_HOST_COHERENT says
    const unsigned hflags = hipHostMallocCoherent | hipHostMallocMapped;
    HIPC(m.pinned(&c->h_pack, (size_t)3 * E * 4, hflags)); HIPC(m.pinned(&c->h_rd, (size_t)2 * E * 4, hflags));
    HIPC(m.dev(&c->d_done_ctr, (size_t)16)); HIPC(m.pinned(&c->h_flag, 64, hflags)); memset(c->h_flag, 0, 64);
    HIPC(m.dev(&c->s_act, (size_t)E)); HIPC(m.dev(&c->s_logp, (size_t)E)); HIPC(m.dev(&c->s_val, (size_t)E));
    for (int k = 0; k < mi_ctx::IDX_RING; ++k) {
        HIPC(m.pinned(&c->h_idx_ring[k], (size_t)NB * sizeof(int32_t), hflags));      // coherent + mapped: a kernel reads it
        HIPC(m.event(&c->idx_ev[k], hipEventDisableTiming));
    }
    c->h_f_floats = (size_t)4 * (E > 64 ? E : 64);
    HIPC(m.pinned(&c->h_f, c->h_f_floats * sizeof(float), hipHostMallocDefault));
    HIPC(m.pinned(&c->h_i, (size_t)E * sizeof(int32_t), hipHostMallocDefault));
    if (getenv("MI355_COPY_GBPS")) c->copy_rate_bytes_per_us = atof(getenv("MI355_COPY_GBPS")) * 1000.0;
    if (c->bf) {
        HIPC(m.dev(&c->fc_wp, (size_t)c->H * 2048)); HIPC(m.dev(&c->fc_wt, (size_t)c->H * 2048));
        HIPC(m.dev(&c->c1_bank, (size_t)conv1_bank_elems()));
        std::vector<BankDesc> desc;
        long long off = 0;
        for (auto& L : c->convs) {
            if (L.cin == 3) continue;                                   // block1.conv stays on the fp32-MFMA kernel
            BankDesc f{L.w_off, off, L.cout, L.cin, L.cout, L.cin, 0, bank_ws(L.cin), L.cin == 32 ? 9 : 5};
            L.bank_f = off; off += (long long)f.rows * f.ws; desc.push_back(f);
            BankDesc d{L.w_off, off, L.cin, L.cout, L.cout, L.cin, 1, bank_ws(L.cout), L.cout == 32 ? 9 : 5};   // dgrad pass: cin_pass = forward cout
            L.bank_d = off; off += (long long)d.rows * d.ws; desc.push_back(d);
        }
        c->n_banks = (int)desc.size();
        HIPC(m.dev(&c->banks, (size_t)off));
        HIPC(m.dev_raw(&c->d_bank_desc, desc.size() * sizeof(BankDesc)));
        HIPC(hipMemcpy(c->d_bank_desc, desc.data(), desc.size() * sizeof(BankDesc), hipMemcpyHostToDevice));
    }
    HIPC(hipDeviceSynchronize());
    return 0;
}

// The one teardown, of a context mi_create could not finish as of a live one.
static void ctx_release(mi_ctx* c) {
    rollout_groups_stop(c);          // the groups' workers joined, then their streams synchronised
    if (c->stream) hipStreamSynchronize(c->stream);
    prof_harvest(c);
    rollout_lanes_return(c);         // (waited for above; the streams go when the last holder of the device returns its lanes)
    mi_comm_destroy(c);
    // Nothing is let go while anything on the device may still read it: the side stream, the null stream's fills and copies and
    // streams of the caller's are not among the waits above.  (The hand-written teardown had this wait implicitly: its first
    // release was a hipFree, which waits for the whole device, in front of every pinned buffer and event; the pool releases
    // newest first, which are pinned buffers and events.)
    hipDeviceSynchronize();
    sae_release(c);
    c->pool.release_all();
    if (c->side_stream) hipStreamDestroy(c->side_stream);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
}
int mi_destroy(mi_ctx* c) { if (c) ctx_release(c); return 0; }

void* mi_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1) != hipSuccess) { g_err = "hipHostMalloc failed"; return nullptr; }
    return p;
}
void mi_host_free(void* p) { if (p) hipHostFree(p); }
// Page-lock caller-owned memory in place (an env's own frame buffer): mi_rollout_submit / mi_put_obs then DMA straight out of it, no
// staging copy on the host.  Fails (-2) where the runtime refuses the range (e.g. pages already registered through another pointer).
int mi_host_register(void* p, size_t bytes) {
    ARG(p && bytes, "null");
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return fail(-2, "hipHostRegister refused the range"); }
    return 0;
}
int mi_host_unregister(void* p) {
    ARG(p, "null");
    if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return fail(-2, "hipHostUnregister failed"); }
    return 0;
}

int mi_sync(mi_ctx* c) { ARG(c, "ctx"); JOIN(c); HIPC(hipStreamSynchronize(c->stream)); return 0; }

int64_t mi_param_count(mi_ctx* c) { return c ? c->n_params : -1; }
int mi_set_params(mi_ctx* c, const float* flat, int64_t n) { ARG(c && flat, "null"); c->fc_packed_valid = false; return upload_flat(c, c->params, flat, n); }
int mi_get_params(mi_ctx* c, float* flat, int64_t n) { ARG(c && flat, "null"); return download_flat(c, c->params, flat, n); }
// PPO.train hands the freshly updated policy to the validation rollouts (agents/ppo.py:241-252 run them with the SAME policy object):
// here the inference-only twin context takes the parameters device to device, in stream order on both sides (no host round trip).
int mi_copy_params(mi_ctx* dst, mi_ctx* src) {
    ARG(dst && src && dst != src, "null / same context"); JOIN(src); JOIN(dst);
    ARG(dst->cfg.arch == src->cfg.arch && dst->n_params == src->n_params && dst->A == src->A && dst->H == src->H && dst->cfg.device == src->cfg.device,
        "contexts of different architecture / size / device");
    hipEvent_t ready = nullptr, done = nullptr;
    DevPool evs(hip_pool());                                        // both events go on every return path (the runtime releases them once they have completed)
    HIPC(evs.event(&ready, hipEventDisableTiming)); HIPC(evs.event(&done, hipEventDisableTiming));
    HIPC(hipEventRecord(ready, src->stream));                      // the optimizer step that wrote src's parameters
    HIPC(hipStreamWaitEvent(dst->stream, ready, 0));
    HIPC(hipMemcpyAsync(dst->params, src->params, (size_t)src->n_params * 4, hipMemcpyDeviceToDevice, dst->stream));
    if (src->gru_train) {          // a trained GRU is part of the policy: the twin acts with the weights the optimizer just wrote
        if (!dst->gru_on) return fail(-1, "invalid argument: the source trains its GRU but the destination has none (mi_set_gru)");
        const GruTensors from = gru_tensors(src), to = gru_tensors(dst);
        for (int k = 0; k < 4; ++k) HIPC(hipMemcpyAsync(to.t[k].p, from.t[k].p, from.t[k].len * 4, hipMemcpyDeviceToDevice, dst->stream));
    }
    HIPC(hipEventRecord(done, dst->stream));
    HIPC(hipStreamWaitEvent(src->stream, done, 0));                // src's next optimizer step must not overtake the copy
    dst->fc_packed_valid = false;                                  // packed bf16 filter images are rebuilt before dst's next pass
    return 0;
}
int mi_get_grads(mi_ctx* c, float* flat, int64_t n) { ARG(c && flat, "null"); return download_flat(c, c->grads, flat, n); }
int mi_set_adam_state(mi_ctx* c, const float* m, const float* v, int64_t n) {
    ARG(c && m && v, "null");
    int r = upload_flat(c, c->adam_m, m, n);
    return r ? r : upload_flat(c, c->adam_v, v, n);
}
int mi_get_adam_state(mi_ctx* c, float* m, float* v, int64_t n) {
    ARG(c && m && v, "null");
    int r = download_flat(c, c->adam_m, m, n);
    return r ? r : download_flat(c, c->adam_v, v, n);
}

// ------------------------------------------------------------------------------------------ rollout storage
int mi_put_obs(mi_ctx* c, int32_t t, const void* obs, size_t bytes) {
    ARG(c && obs, "null"); JOIN(c); ARG(t >= 0 && t <= c->T, "t out of range");
    const size_t want = (size_t)c->E * c->obs_bytes_per_env;
    ARG(bytes == want, "obs byte count != E * bytes_per_env");
    HIPC(hipMemcpyAsync(obs_ring(c) + (size_t)t * want, obs, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}
int mi_get_obs(mi_ctx* c, int32_t t, void* obs, size_t bytes) {
    ARG(c && obs, "null"); JOIN(c); ARG(t >= 0 && t <= c->T, "t out of range");
    const size_t want = (size_t)c->E * c->obs_bytes_per_env;
    ARG(bytes == want, "obs byte count != E * bytes_per_env");
    HIPC(hipMemcpyAsync(obs, obs_ring(c) + (size_t)t * want, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_put_step(mi_ctx* c, int32_t t, const float* rew, const float* done) {
    ARG(c && rew && done, "null"); JOIN(c); ARG(t >= 0 && t < c->T, "t out of range");
    const size_t b = (size_t)c->E * sizeof(float);
    HIPC(hipMemcpyAsync(c->rew + (size_t)t * c->E, rew, b, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->done + (size_t)t * c->E, done, b, hipMemcpyHostToDevice, c->stream));
    return 0;
}
int mi_put_policy_outputs(mi_ctx* c, int32_t t, const int32_t* act, const float* logp, const float* value) {
    ARG(c, "null"); JOIN(c); ARG(t >= 0 && t <= c->T, "t out of range");
    const size_t E = c->E;
    if (act) { ARG(t < c->T, "act at t==T"); HIPC(hipMemcpyAsync(c->act + t * E, act, E * 4, hipMemcpyHostToDevice, c->stream)); }
    if (logp) { ARG(t < c->T, "logp at t==T"); HIPC(hipMemcpyAsync(c->logp + t * E, logp, E * 4, hipMemcpyHostToDevice, c->stream)); }
    if (value) HIPC(hipMemcpyAsync(c->value + t * E, value, E * 4, hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));     // caller buffers may be pageable temporaries
    return 0;
}
static float* field_ptr(mi_ctx* c, int f, int64_t* n) {
    const int64_t TE = (int64_t)c->T * c->E;
    *n = TE;
    switch (f) {
        case MI_F_REW: return c->rew; case MI_F_DONE: return c->done; case MI_F_LOGP: return c->logp;
        case MI_F_ADV: return c->adv; case MI_F_RET: return c->ret;
        case MI_F_VALUE: *n = TE + c->E; return c->value;
        default: return nullptr;
    }
}
int mi_read_field(mi_ctx* c, int32_t f, float* out, int64_t n) {
    ARG(c && out, "null"); JOIN(c);
    if (f == MI_F_ACT) {
        ARG(n == (int64_t)c->T * c->E, "length");
        std::vector<int32_t> tmp(n);
        HIPC(hipMemcpyAsync(tmp.data(), c->act, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        for (int64_t k = 0; k < n; ++k) out[k] = (float)tmp[k];
        return 0;
    }
    int64_t want; float* p = field_ptr(c, f, &want);
    ARG(p, "field"); ARG(n == want, "length");
    HIPC(hipMemcpyAsync(out, p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_write_field(mi_ctx* c, int32_t f, const float* in, int64_t n) {
    ARG(c && in, "null"); JOIN(c);
    if (f == MI_F_ACT) {
        ARG(n == (int64_t)c->T * c->E, "length");
        std::vector<int32_t> tmp(n);
        for (int64_t k = 0; k < n; ++k) tmp[k] = (int32_t)in[k];
        HIPC(hipMemcpyAsync(c->act, tmp.data(), n * 4, hipMemcpyHostToDevice, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        return 0;
    }
    int64_t want; float* p = field_ptr(c, f, &want);
    ARG(p, "field"); ARG(n == want, "length");
    HIPC(hipMemcpyAsync(p, in, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------ profiler
static hipEvent_t prof_event(mi_ctx* c) {
    hipEvent_t e = nullptr;
    if (!c->prof.pool.empty()) { e = c->prof.pool.back(); c->prof.pool.pop_back(); return e; }
    c->prof.made.emplace_back();                 // (a deque: the context's pool keeps the address of what it hands out)
    c->pool.event(&c->prof.made.back(), hipEventDefault);
    return c->prof.made.back();
}
static void prof_harvest(mi_ctx* c) {
    if (c->prof.pend.empty()) return;
    hipStreamSynchronize(c->stream);
    for (const RolloutGroup& G : c->grp) if (G.stream) hipStreamSynchronize(G.stream);
    for (auto& p : c->prof.pend) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, p.a, p.b);
        c->prof.ms[p.phase][p.cls] += ms; c->prof.launches[p.phase][p.cls]++; c->prof.units[p.phase][p.cls] += p.units;
        c->prof.bytes[p.phase][p.cls] += p.bytes; c->prof.flops[p.phase][p.cls] += p.flops;
        c->prof.pool.push_back(p.a); c->prof.pool.push_back(p.b);
    }
    c->prof.pend.clear();
}
struct ProfScope {
    mi_ctx* c; ProfPending p; bool live;
    // bytes / flops: ALGORITHMIC figures of this launch (layer-boundary model)
    ProfScope(mi_ctx* c_, int cls, long long units, double bytes, double flops, bool enable = true)
        : c(c_), live(enable && !tl_stream && c_->prof.on && (c_->prof.phase == 1 ? c_->prof.sample_now : c_->prof.all_phases)) {
        if (!live) return;
        p.a = prof_event(c); p.b = prof_event(c); p.cls = cls; p.phase = c->prof.phase; p.units = units; p.bytes = bytes; p.flops = flops;
        hipEventRecord(p.a, c->stream);
    }
    ~ProfScope() {
        if (!live) return;
        hipEventRecord(p.b, c->stream);
        c->prof.pend.push_back(p);
        if (c->prof.pend.size() >= 4096) prof_harvest(c);
    }
};
int mi_profile_enable(mi_ctx* c, int32_t enabled) {
    ARG(c, "null");
    if (!enabled) prof_harvest(c);
    c->prof.on = (enabled & 0xff) != 0; c->prof.all_phases = (enabled & 0xff) == 2;
    c->prof.period = (enabled >> 8) > 0 ? (enabled >> 8) : 1; c->prof.mb_count = 0; c->prof.sample_now = true;
    return 0;
}
const char* mi_profile_class_name(int32_t id) { return (id >= 0 && id < PC_COUNT) ? kProfNames[id] : ""; }
int mi_profile_read(mi_ctx* c, double* rows, int32_t max_rows, int32_t* n_rows, int32_t reset) {
    ARG(c && rows && n_rows, "null"); JOIN(c);
    prof_harvest(c);
    int n = 0;
    for (int ph = 0; ph < 2; ++ph)
        for (int k = 0; k < PC_COUNT; ++k)
            if (c->prof.launches[ph][k] > 0 && n < max_rows) {
                double* r = rows + (size_t)n * 7;
                r[0] = k; r[1] = ph; r[2] = (double)c->prof.launches[ph][k]; r[3] = c->prof.ms[ph][k]; r[4] = (double)c->prof.units[ph][k];
                r[5] = c->prof.bytes[ph][k]; r[6] = c->prof.flops[ph][k];
                ++n;
            }
    *n_rows = n;
    if (reset) { memset(c->prof.ms, 0, sizeof(c->prof.ms)); memset(c->prof.launches, 0, sizeof(c->prof.launches)); memset(c->prof.units, 0, sizeof(c->prof.units));
                 memset(c->prof.bytes, 0, sizeof(c->prof.bytes)); memset(c->prof.flops, 0, sizeof(c->prof.flops)); }
    return 0;
}

// ------------------------------------------------------------------------------------------ network program
static void conv_fwd(mi_ctx* c, const ConvLayer& L, const void* in, const InputSrc* src, int relu_in, const float* res, float* out, int n) {
    ConvArgs a{};
    a.in = src ? src->base : in; a.idx = src ? src->idx : nullptr; a.in_base = src ? src->first : 0;
    a.w = c->params + L.w_off; a.bias = c->params + L.b_off; a.res = res; a.mask = nullptr; a.out = out;
    a.lut = c->lut; a.n = n; a.relu_in = relu_in; a.bf16 = c->bf;
    a.wbank = (c->bf && L.bank_f >= 0) ? c->banks + L.bank_f : nullptr;
    a.lut16 = c->bf ? c->lut16 : nullptr;
    const double px = (double)n * L.hw * L.hw, es = c->es;
    ProfScope ps(c, PC_CONV_FWD + (int)L.shape, n, px * ((L.cin == 3 ? 3.0 : es * L.cin) + es * L.cout * (res ? 2 : 1)), px * 18.0 * L.cin * L.cout);
    launch_conv_fwd(L.shape, a, CUR(c));
}
static void conv_dgrad(mi_ctx* c, const ConvLayer& L, const float* dout, const float* mask, const float* res, float* din, int n, const uint8_t* pool_arg = nullptr) {
    ConvArgs a{};
    a.pool_arg = pool_arg;
    a.in = dout; a.w = c->params + L.w_off; a.bias = nullptr; a.res = res; a.mask = mask; a.out = din;
    a.lut = c->lut; a.n = n; a.relu_in = 0; a.bf16 = c->bf;
    a.wbank = (c->bf && L.bank_d >= 0) ? c->banks + L.bank_d : nullptr;
    const double px = (double)n * L.hw * L.hw;
    const double pool_b = pool_arg ? c->es * (px / 4 * L.cout + 2.0 * px * L.cout) : 0.0;      // POOLIN: the max-pool backward (p + 2X of SURVEY 8(d)) rides along
    ProfScope ps(c, PC_CONV_DGRAD + (int)L.shape, n, px * c->es * (L.cout + L.cin * (1 + (mask ? 1 : 0) + (res ? 1 : 0))) + pool_b, px * 18.0 * L.cin * L.cout);
    launch_conv_dgrad(L.shape, a, CUR(c));
}
// layer's weight-gradient slabs [grid][wlen + cout] join the table that ONE launch sums at the end of net_backward (conv_wgrad_reduce_all)
static inline void push_slab(mi_ctx* c, int layer, int grid) {
    const ConvLayer& L = c->convs[layer];
    const int wlen = L.cout * 9 * L.cin;
    c->h_slab_desc[c->slab_desc_n++] = SlabDesc{c->slab_off[layer], (long long)L.w_off, (long long)L.b_off, grid, wlen + L.cout, wlen};
}
static void conv_wgrad(mi_ctx* c, const ConvLayer& L, const void* in, const InputSrc* src, int relu_in, const float* dout, int n, const uint8_t* pool_arg = nullptr) {
    WgradArgs a{};
    a.pool_arg = pool_arg;
    a.in = src ? src->base : in; a.idx = src ? src->idx : nullptr; a.in_base = src ? src->first : 0;
    const int layer = (int)(&L - c->convs.data());
    a.dout = dout; a.partial = c->slabs + c->slab_off[layer]; a.lut = c->lut; a.n = n; a.relu_in = relu_in; a.bf16 = c->bf;
    a.lut16 = c->bf ? c->lut16 : nullptr;
    const int grid = wgrad_grid_for(L.shape, n, c->bf);
    if (grid < 1) return;
    if (grid > 1024) { net_err_set(c, "weight-gradient launch needs more than the 1024 slabs a layer owns"); return; }
    const double px = (double)n * L.hw * L.hw;
    { // SURVEY 8(d) layer-boundary bytes; block1.conv from the pooled gradient also carries the max-pool backward (p + 2X)
      const double pool_b = (pool_arg && L.cin == 3) ? c->es * (px / 4 * L.cout + 2.0 * px * L.cout) : 0.0;
      ProfScope ps(c, PC_CONV_WGRAD + (int)L.shape, n, px * ((L.cin == 3 ? 3.0 : c->es * L.cin) + c->es * L.cout) + pool_b, px * 18.0 * L.cin * L.cout);
      launch_conv_wgrad(L.shape, a, CUR(c)); }
    push_slab(c, layer, grid);
}
// Gradient all-reduce of an ARMED backward pass (mi_allreduce_arm): a region of the flat gradient goes to the side stream as soon as
// the main stream has written it for the last time.  Region A = [fc.weight .. end) (embedder.fc + heads: 84 % of the parameters, final
// right after the first three launches of the backward pass, so their exchange hides behind the whole conv stack's backward);
// region B = [0, fc.weight) (the 15 conv layers: final only once the per-workgroup slabs are summed, at the very end).
static void issue_grad_allreduce(mi_ctx* c, int64_t off, int64_t n, bool last) {
    if (!c->ar_armed || !c->comm || n <= 0) return;
    hipEventRecord(c->ev_ar_ready, CUR(c));
    hipStreamWaitEvent(c->comm_stream, c->ev_ar_ready, 0);
    ncclResult_t r = ncclAllReduce(c->grads + off, c->grads + off, (size_t)n, ncclFloat, ncclSum, c->comm_grad, c->comm_stream);
    if (r != ncclSuccess) { net_err_set(c, std::string("ncclAllReduce (gradients): ") + ncclGetErrorString(r)); return; }
    if (last) { hipEventRecord(c->ev_ar_done, c->comm_stream); c->ar_armed = false; c->ar_issued = true; c->ar_inflight = true; }
}

static void conv_wgrad_reduce_all(mi_ctx* c, int n, int first = 0) {          // first: entries [0, first) are summed already (net_backward's second fork)
    if (c->slab_desc_n <= 0) return;
    int max_len = 0; double bytes = 0;
    for (int k = first; k < c->slab_desc_n; ++k) { max_len = std::max(max_len, c->h_slab_desc[k].slab_len); bytes += 4.0 * c->h_slab_desc[k].nslab * c->h_slab_desc[k].slab_len; }
    // the descriptor table only depends on the batch size: re-uploaded when it changes (pageable source copied at call time)
    if (c->slab_desc_cached_n != n) {
        hipMemcpyAsync(c->d_slab_desc, c->h_slab_desc, sizeof(SlabDesc) * c->slab_desc_n, hipMemcpyHostToDevice, CUR(c));
        c->slab_desc_cached_n = n;
    }
    { ProfScope ps(c, PC_SLAB_REDUCE, n, bytes, 0.0);
      launch_reduce_all_slabs(c->slabs, c->grads, c->d_slab_desc + first, c->slab_desc_n - first, max_len, CUR(c)); }
    c->slab_desc_n = 0;
}

void linear_fwd(mi_ctx* c, const float* X, int relu_x, const float* W, const float* b, float* Y, int n, int in, int out, int relu_out, int x_bf16) {
    GemmArgs g{};
    const GemmWs ws = gemm_ws(c); g.ws = ws.p; g.ws_floats = ws.floats;
    g.a_bf16 = x_bf16;
    g.A = X; g.B = W; g.C = Y; g.M = n; g.N = out; g.K = in;
    g.sam = in; g.sak = 1; g.sbk = 1; g.sbn = in; g.ldc = out;
    g.bias = b; g.relu_a = relu_x; g.relu_out = relu_out;
    ProfScope ps(c, PC_GEMM, n, 4.0 * ((double)n * in + (double)in * out + (double)n * out), 2.0 * n * in * out);
    launch_gemm(g, CUR(c));
}
// dX = dY W  (* mask > 0)
void linear_dgrad(mi_ctx* c, const float* dY, const float* W, const float* mask, float* dX, int n, int in, int out, int x_bf16) {
    GemmArgs g{};
    const GemmWs ws = gemm_ws(c); g.ws = ws.p; g.ws_floats = ws.floats;
    g.mask_bf16 = x_bf16; g.c_bf16 = x_bf16;          // mask source and dX are activation-typed
    g.A = dY; g.B = W; g.C = dX; g.M = n; g.N = in; g.K = out;
    g.sam = out; g.sak = 1; g.sbk = in; g.sbn = 1; g.ldc = in; g.mask = mask;
    ProfScope ps(c, PC_GEMM, n, 4.0 * ((double)n * out + (double)in * out + (double)n * in * (mask ? 2 : 1)), 2.0 * n * in * out);
    launch_gemm(g, CUR(c));
}
// gW += dY^T relu?(X) ; gb += colsum(dY)
void linear_wgrad(mi_ctx* c, const float* dY, const float* X, int relu_x, float* gW, float* gb, int n, int in, int out, int x_bf16) {
    GemmArgs g{};
    const GemmWs ws = gemm_ws(c); g.ws = ws.p; g.ws_floats = ws.floats;
    g.b_bf16 = x_bf16;
    g.A = dY; g.B = X; g.C = gW; g.M = out; g.N = in; g.K = n;
    g.sam = 1; g.sak = out; g.sbk = in; g.sbn = 1; g.ldc = in; g.relu_b = relu_x; g.accumulate = 1;
    ProfScope ps(c, PC_GEMM, n, 4.0 * ((double)n * out + (double)n * in + (double)in * out), 2.0 * n * in * out);
    launch_gemm(g, CUR(c));
    launch_colsum_acc(dY, n, out, out, gb, c->col_ws, CUR(c));
}

static void net_heads(mi_ctx* c, int n, int soff = 0) {
    // (tests/test_gpu_lse_value.py::test_update_sized_heads_and_partial_loss_block picks its 1040 samples to be past this threshold)
    if (c->H == 256 && c->A + 1 <= 16 && n >= 1024) {      // update-sized batches: dedicated kernel (heads.hip heads_fwd_kernel)
        ProfScope ps(c, PC_GEMM, n, 4.0 * ((double)n * c->H + (double)n * (c->A + 1) + (double)c->H * (c->A + 1)), 2.0 * n * c->H * (c->A + 1));
        launch_heads_fwd(c->feat + (size_t)soff * c->H, c->params + c->wh_off, c->params + c->bh_off, c->hout + (size_t)soff * (c->A + 1), n, c->A + 1, CUR(c));
        return;
    }
    linear_fwd(c, c->feat + (size_t)soff * c->H, 0, c->params + c->wh_off, c->params + c->bh_off, c->hout + (size_t)soff * (c->A + 1), n, c->H, c->A + 1, 0);
}
// h' = GRU(feat, h_state * (1 - done)); feat <- h' ; h_state <- h'   (n == E rows)
static void net_gru(mi_ctx* c, int n, int soff, bool keep_x) {
    const int H = c->H;
    const size_t o = (size_t)soff * H;
    launch_mask_rows(c->h_state + o, c->d_done + soff, c->h_masked + o, n, H, CUR(c));
    linear_fwd(c, c->feat + o, 0, c->gru_wih, c->gru_bih, c->gru_gi + 3 * o, n, H, 3 * H, 0);
    linear_fwd(c, c->h_masked + o, 0, c->gru_whh, c->gru_bhh, c->gru_gh + 3 * o, n, H, 3 * H, 0);
    if (keep_x) hipMemcpyAsync(c->gru_x + o, c->feat + o, (size_t)n * H * 4, hipMemcpyDeviceToDevice, CUR(c));     // (the gates kernel overwrites feat with h')
    launch_gru_gates(c->gru_gi + 3 * o, c->gru_gh + 3 * o, c->h_masked + o, c->h_state + o, c->feat + o, n, H, CUR(c));
}

void fc_refresh(mi_ctx* c) {
    if (c->bf && !c->fc_packed_valid) {
        launch_repack_all(c->params, c->banks, c->d_bank_desc, c->n_banks, c->convs.empty() ? nullptr : c->params + c->convs[0].w_off,
                          c->convs.empty() ? nullptr : c->c1_bank, c->params + c->fc.w_off, c->fc_wp, c->fc_wt, c->H, CUR(c));
        c->fc_packed_valid = true;
    }
}

// ---- forward, one function per mode: each is the launch list of a pass from the observations to feat (n x H)
// block b's buffers from row soff on (element size: c->es bytes; arg-max: 1 byte)
static Block block_view(const mi_ctx* c, int b, int soff) {
    Block k = c->blk[b];
    if (soff) {
        const size_t pe = (size_t)(k.hin / 2) * (k.hin / 2) * k.cout, po = (size_t)soff * pe * (size_t)c->es;
        auto sh = [&](float* q, size_t bytes) { return q ? (float*)((char*)q + bytes) : q; };
        k.C = sh(k.C, po * 4); k.P0 = sh(k.P0, po); k.A1 = sh(k.A1, po); k.P1 = sh(k.P1, po); k.A2 = sh(k.A2, po); k.P2 = sh(k.P2, po);
        k.PI += (size_t)soff * pe;
    }
    return k;
}

static void forward_mlp(mi_ctx* c, const InputSrc& src, int n, int soff, float* feat) {
    float* x0 = c->mlp_act[0] + (size_t)soff * c->cfg.obs_dim;
    launch_gather_rows((const float*)src.base, src.idx, src.first, x0, n, c->cfg.obs_dim, CUR(c));
    const size_t L = c->mlp.size();
    const float* x = x0;
    for (size_t l = 0; l < L; ++l) {
        float* y = (l + 1 == L) ? feat : c->mlp_act[l + 1] + (size_t)soff * c->mlp[l].out;
        linear_fwd(c, x, 0, c->params + c->mlp[l].w_off, c->params + c->mlp[l].b_off, y, n, c->mlp[l].in, c->mlp[l].out, l + 1 < L);
        x = y;
    }
}

static void forward_impala_fp32(mi_ctx* c, const InputSrc& src, int n, int soff, float* feat) {
    const float* prev = nullptr;
    for (int b = 0; b < 3; ++b) {
        const Block k = block_view(c, b, soff);
        const ConvLayer* L = &c->convs[b * 5];
        if (b == 0) conv_fwd(c, L[0], nullptr, &src, 0, nullptr, k.C, n);
        else conv_fwd(c, L[0], prev, nullptr, 0, nullptr, k.C, n);
        { ProfScope ps(c, PC_POOL_FWD, n, (double)n * k.hin * k.hin * k.cout * (c->es * 1.25 + 0.25), 0.0);
          launch_maxpool_fwd(k.C, k.P0, k.PI, n, k.hin, k.cout, CUR(c)); }
        conv_fwd(c, L[1], k.P0, nullptr, 1, nullptr, k.A1, n);
        conv_fwd(c, L[2], k.A1, nullptr, 1, k.P0, k.P1, n);
        conv_fwd(c, L[3], k.P1, nullptr, 1, nullptr, k.A2, n);
        conv_fwd(c, L[4], k.A2, nullptr, 1, k.P1, k.P2, n);
        prev = k.P2;
    }
    linear_fwd(c, prev, 1, c->params + c->fc.w_off, c->params + c->fc.b_off, feat, n, 2048, c->H, 1, 0);
}

// false: a launch was refused (reported through net_err) and the pass stops
static bool forward_impala_bf16(mi_ctx* c, const InputSrc& src, int n, int soff, float* feat, bool train) {
    // rollout-sized inference batches: blocks 2 and 3 in ONE launch, one workgroup per image (rollout_bf16.hip)
    const bool fused_tail = !train && n <= 256 && c->rollout_tail;
    const float* prev = nullptr;
    for (int b = 0; b < 3; ++b) {
        const Block k = block_view(c, b, soff);
        const ConvLayer* L = &c->convs[b * 5];
        if (fused_tail && b == 1) {
            const unsigned short* bk[10]; const float* bb[10];
            for (int q = 0; q < 10; ++q) { bk[q] = c->banks + c->convs[5 + q].bank_f; bb[q] = c->params + c->convs[5 + q].b_off; }
            const Block k3 = block_view(c, 2, soff);
            { const double px2 = (double)n * 32 * 32, px3 = (double)n * 16 * 16;
              ProfScope ps(c, PC_RESBLOCK + (int)CS_32_32_16, n, 2.0 * (px2 * 16 + px3 / 4 * 32), px2 * 18.0 * 16 * 32 + 5.0 * px3 * 18.0 * 32 * 32 + 4.0 * (px3 / 4) * 18.0 * 32 * 32);
              launch_rollout_tail_bf16(prev, k3.P2, n, bk, bb, CUR(c)); }
            prev = k3.P2;
            break;
        }
        if (b == 0) {           // block1.conv + max pool fused: the 64x64x16 conv output never reaches HBM
            ConvArgs a{};
            a.in = src.base; a.idx = src.idx; a.in_base = src.first; a.w = c->params + L[0].w_off; a.bias = c->params + L[0].b_off;
            a.n = n; a.bf16 = 1; a.lut16 = c->lut16; a.wbank = c->c1_bank;
            const double px = (double)n * 64 * 64;
            ProfScope ps(c, PC_CONV_FWD + (int)L[0].shape, n, px * 3.0 + 2.0 * (2.0 * px * 16 + px / 4 * 16), px * 18.0 * 3 * 16);      // conv I + X, pool X + p
            launch_conv1_pool_fwd_bf16(a, c->lut16, k.P0, k.PI, CUR(c));
        } else {                // block2.conv / block3.conv + max pool fused as well (convpool_bf16.hip)
            ConvArgs a{};
            a.in = prev; a.bias = c->params + L[0].b_off; a.n = n; a.bf16 = 1; a.wbank = c->banks + L[0].bank_f;
            const double px = (double)n * L[0].hw * L[0].hw;
            ProfScope ps(c, PC_CONV_FWD + (int)L[0].shape, n, 2.0 * (px * L[0].cin + 2.0 * px * L[0].cout + px / 4 * L[0].cout), px * 18.0 * L[0].cin * L[0].cout);      // 8(d): I + 2X + p
            if (!launch_conv_pool_fwd_bf16(L[0].shape, a, k.P0, k.PI, CUR(c))) { net_err_set(c, "no fused conv+pool kernel for this conv shape"); return false; }
        }
        {                       // res1 + res2 in ONE launch; intermediates reach HBM only when a backward pass follows
            const double px = (double)n * L[1].hw * L[1].hw, ch = L[1].cout;
            const float* bb[4] = {c->params + L[1].b_off, c->params + L[2].b_off, c->params + L[3].b_off, c->params + L[4].b_off};
            const unsigned short* bk[4] = {c->banks + L[1].bank_f, c->banks + L[2].bank_f, c->banks + L[3].bank_f, c->banks + L[4].bank_f};
            ProfScope ps(c, PC_RESBLOCK + (int)L[1].shape, n, px * ch * 2.0 * 10, 4.0 * px * 18.0 * ch * ch);      // 8(d): 2 blocks x (2 convs x 2p + skip p) = 10p (the kernel itself moves 5p)
            launch_resblock_pair_bf16(L[1].shape, k.P0, bb, train ? k.A1 : nullptr, train ? k.P1 : nullptr, train ? k.A2 : nullptr, k.P2, n, bk, CUR(c));
        }
        prev = k.P2;
    }
    {                           // bf16 matrix cores on the packed [H][2048] weight image (fc_bf16.hip)
        const double H = c->H;
        ProfScope ps(c, PC_GEMM, n, 2.0 * n * 2048 + 2.0 * 2048 * H + 4.0 * n * H, 2.0 * n * 2048 * H);
        if (n >= 1024) launch_fc_fwd_bf16(prev, c->fc_wp, c->params + c->fc.b_off, feat, n, c->H, CUR(c));
        else launch_fc_fwd_small_bf16(prev, c->fc_wp, c->params + c->fc.b_off, feat, n, c->H, CUR(c));   // rollout-sized: latency-bound
    }
    return true;
}

void net_forward(mi_ctx* c, const InputSrc& src, int n, const FwdOpts& o) {
    fc_refresh(c);          // bf16 mode: packed fc / conv filter images follow the parameters
    float* const feat = c->feat + (size_t)o.soff * c->H;
    if (c->cfg.arch != MI_ARCH_IMPALA) forward_mlp(c, src, n, o.soff, feat);
    else if (!c->bf) forward_impala_fp32(c, src, n, o.soff, feat);
    else if (!forward_impala_bf16(c, src, n, o.soff, feat, o.train)) return;
    if (o.recurrent && c->gru_on) net_gru(c, n, o.soff, o.keep_gru_x);
    if (o.heads) net_heads(c, n, o.soff);
}

// ---- backward
// The heads' three gradients from dY (n x (A+1)).  fused (each caller's own condition): one launch (heads.hip heads_bwd_kernel) that also sums
// its slabs unless the side stream of a forking pass does (with_reduce false; it forks on done_ev = this launch's own completion); else two GEMMs + a
// column sum.  prof: only net_backward's launch is bracketed for the profiler.
static void heads_backward(mi_ctx* c, int n, int relu_mask, bool fused, bool prof, hipStream_t st, bool with_reduce = true, hipEvent_t done_ev = nullptr) {
    if (fused) {
        ProfScope ps(c, PC_GEMM, n, 4.0 * ((double)n * (c->A + 1) + 2.0 * n * c->H + (double)c->H * (c->A + 1)), 4.0 * n * c->H * (c->A + 1), prof);
        launch_heads_bwd(c->dY, c->feat, c->params + c->wh_off, relu_mask, c->dfeat, c->grads + c->wh_off, c->grads + c->bh_off, c->gemm_ws, n, c->H, c->A + 1, st, with_reduce, done_ev);
        return;
    }
    linear_wgrad(c, c->dY, c->feat, 0, c->grads + c->wh_off, c->grads + c->bh_off, n, c->H, c->A + 1);
    linear_dgrad(c, c->dY, c->params + c->wh_off, relu_mask ? c->feat : nullptr, c->dfeat, n, c->H, c->A + 1);
}

// backward_*: the embedder's backward pass from dfeat.  Each returns where it left the gradient of the first layer's output (the MLP's first
// linear layer; IMPALA fp32: block1.conv; bf16: block 1's max pool), which the value saliency takes on to the observation.
static const float* backward_mlp(mi_ctx* c, int n) {
    const size_t L = c->mlp.size();
    const float* dy = c->dfeat;
    for (size_t l = L; l-- > 0;) {
        linear_wgrad(c, dy, c->mlp_act[l], 0, c->grads + c->mlp[l].w_off, c->grads + c->mlp[l].b_off, n, c->mlp[l].in, c->mlp[l].out);
        if (l == 0) break;
        float* dx = c->GP[l & 1];
        linear_dgrad(c, dy, c->params + c->mlp[l].w_off, c->mlp_act[l], dx, n, c->mlp[l].in, c->mlp[l].out);
        dy = dx;
    }
    issue_grad_allreduce(c, 0, c->n_params, true);
    return L ? dy : nullptr;
}

// + fs_coef * d(feature sparsity) / d(block3 output): one element per column (launch_fs_grad, loss.hip)
static void fs_gradient(mi_ctx* c, int n, float* G, const BwdOpts& o) {
    if (o.fs_coef == 0.f) return;
    if (o.fs_from_keys) { if (n > 0) launch_fs_apply_keys(G, c->bf, 2048, c->fs_keys, c->fs_keys_local, c->fs_arg, o.fs_coef, CUR(c)); }      // the column's winner among the ranks
    else launch_fs_grad(c->blk[2].P2, c->bf, n, 2048, c->fs_scratch, o.fs_groups, G, o.fs_coef, c->fs_colmax, c->fs_arg, CUR(c));
}

static const float* backward_impala_fp32(mi_ctx* c, const InputSrc& src, int n, const BwdOpts& o) {
    linear_wgrad(c, c->dfeat, c->blk[2].P2, 1, c->grads + c->fc.w_off, c->grads + c->fc.b_off, n, 2048, c->H, 0);
    issue_grad_allreduce(c, c->fc.w_off, c->n_params - c->fc.w_off, false);       // region A: fc + heads gradients are final
    float *Gout = c->GP[0], *Ga = c->GP[1], *Gb = c->GP[2];
    linear_dgrad(c, c->dfeat, c->params + c->fc.w_off, c->blk[2].P2, Gout, n, 2048, c->H, 0);
    fs_gradient(c, n, Gout, o);
    for (int b = 2; b >= 0; --b) {
        Block& k = c->blk[b];
        const ConvLayer* L = &c->convs[b * 5];
        // res2: P2 = conv2(relu(A2)) + P1 ; A2 = conv1(relu(P1))
        conv_wgrad(c, L[4], k.A2, nullptr, 1, Gout, n);
        conv_dgrad(c, L[4], Gout, k.A2, nullptr, Ga, n);
        conv_wgrad(c, L[3], k.P1, nullptr, 1, Ga, n);
        conv_dgrad(c, L[3], Ga, k.P1, Gout, Gb, n);
        // res1: P1 = conv2(relu(A1)) + P0 ; A1 = conv1(relu(P0))
        conv_wgrad(c, L[2], k.A1, nullptr, 1, Gb, n);
        conv_dgrad(c, L[2], Gb, k.A1, nullptr, Ga, n);
        conv_wgrad(c, L[1], k.P0, nullptr, 1, Ga, n);
        conv_dgrad(c, L[1], Ga, k.P0, Gb, Gout, n);
        // max pool, then the block's first conv
        { ProfScope ps(c, PC_POOL_BWD, n, (double)n * k.hin * k.hin * k.cout * (c->es * 1.25 + 0.25), 0.0);
          launch_maxpool_bwd(Gout, k.PI, c->GC, n, k.hin, k.cout, CUR(c)); }
        if (b == 0) conv_wgrad(c, L[0], nullptr, &src, 0, c->GC, n);
        else {
            conv_wgrad(c, L[0], c->blk[b - 1].P2, nullptr, 0, c->GC, n);
            conv_dgrad(c, L[0], c->GC, nullptr, nullptr, Gout, n);
        }
    }
    conv_wgrad_reduce_all(c, n);
    issue_grad_allreduce(c, 0, c->fc.w_off, true);                                 // region B: the conv layers' gradients
    return c->GC;
}

// First fork of a bf16 pass, behind heads_bwd: the side stream takes the logged statistics and embedder.fc's weight / bias gradients
// (mi_ctx::side_stream); the main stream goes straight on to the data gradient.  Every buffer the side work touches (block-3 output, feat,
// dfeat, loss partial sums, the split-K / column-sum / metric workspaces, the fc + head slices of grads) is next written after the join.
static void fork_stats_and_fc(mi_ctx* c, int n, const SideJob& j) {
    fc_refresh(c);
    hipStream_t ss = side_stream(c);
    hipStreamWaitEvent(ss, c->ev_side_fork, 0);          // (recorded at heads_bwd_kernel's own completion: heads_backward in net_backward)
    if (j.idx_slot >= 0) hipEventRecord(c->idx_ev[j.idx_slot], ss);      // (stage_indices: the index slot's "read" marker)
    tl_stream = ss;
    launch_heads_bwd_reduce(c->gemm_ws, c->grads + c->wh_off, c->grads + c->bh_off, n, c->H, c->A + 1, ss);      // (before fc_tn reuses the slabs)
    launch_fs_metric_seg(c->blk[2].P2, c->bf, j.st, 2048, c->fs_scratch, c->fs_parts, ss);
    launch_loss_finalize_seg(j.a, j.st, j.mode, j.ring, c->fs_parts, 2048, j.fsr, j.log, ss);
    launch_fc_tn(c->dfeat, (const unsigned short*)c->blk[2].P2, c->grads + c->fc.w_off, c->gemm_ws, (size_t)8 << 20, c->H, 2048, n, ss);
    launch_colsum_acc(c->dfeat, n, c->H, c->H, c->grads + c->fc.b_off, c->col_ws, ss);
    tl_stream = nullptr;
    hipEventRecord(c->ev_side_join, ss);
}
// Second fork, in front of block1.conv's weight gradient: that is the last kernel of the pass and nothing but its own slabs depends on it,
// so the slab sums of the 14 layers before it run beside it (the table on the device is the cached one of this batch size: its last entry
// is block1.conv's) and only that last entry is summed behind it.  Returns the number of table entries summed here.
static int fork_slab_sums(mi_ctx* c, bool fork_recorded) {
    hipStream_t ss = side_stream(c);
    int max_len = 0;
    for (int q = 0; q < c->slab_desc_n; ++q) max_len = std::max(max_len, c->h_slab_desc[q].slab_len);
    if (!fork_recorded) hipEventRecord(c->ev_side_fork, c->stream);
    hipStreamWaitEvent(ss, c->ev_side_fork, 0);
    launch_reduce_all_slabs(c->slabs, c->grads, c->d_slab_desc, c->slab_desc_n, max_len, ss);
    hipEventRecord(c->ev_side_join, ss);
    return c->slab_desc_n;
}

// Both residual blocks of block b, bf16: the gradient of the block's output arrives in G and the gradient of its pooled map leaves in G
// (Ga, Gb: scratch).  done_ev, if set, is to be recorded at the completion of the pair's last launch; returns whether a launch took it.
static bool backward_residual_pair(mi_ctx* c, int b, int n, float* G, float* Ga, float* Gb, hipEvent_t done_ev) {
    const Block& k = c->blk[b];
    const ConvShape s = c->convs[b * 5 + 1].shape;
    const double px = (double)n * c->convs[b * 5 + 1].hw * c->convs[b * 5 + 1].hw, ch = c->convs[b * 5 + 1].cout;
    bool ev_taken = false;
    // one residual block y = conv2(relu(a)) + x, a = conv1(relu(x)) (conv1 = layer i1, conv2 = layer i1 + 1): dy -> dx, both weight gradients
    auto residual = [&](int i1, const float* dy, const float* a_fwd, const float* x_fwd, float* dx, hipEvent_t ev) {
        const int i2 = i1 + 1;
        const ConvLayer &l1 = c->convs[i1], &l2 = c->convs[i2];
        const unsigned short *bank2 = c->banks + l2.bank_d, *bank1 = c->banks + l1.bank_d;
        if (s == CS_16_16_32 || s == CS_32_32_16 || s == CS_32_32_8) {
            // data gradients AND both weight gradients in one launch; the gradient of conv1's output never reaches HBM.  16 channels @32x32:
            // resblock_bwd_full16d_bf16_kernel; 32 channels @16x16: resblock_bwd_full32s_bf16_kernel, @8x8: resblock_bwd_full32q_bf16_kernel
            const bool c16 = s == CS_16_16_32;
            const int grid = c16 ? resblock_bwd_full_grid(n) : resblock_bwd_full32_grid(s, n);
            float *slab2 = c->slabs + c->slab_off[i2], *slab1 = c->slabs + c->slab_off[i1];
            { ProfScope ps(c, PC_RESBLOCK_BWD + (int)s, n, px * ch * 2.0 * 7, 4.0 * px * 18.0 * ch * ch);      // 8(d): 2 convs x 3p + skip-gradient p = 7p (the kernel itself moves 4p)
              if (c16) launch_resblock_bwd_full_bf16(dy, a_fwd, x_fwd, dx, nullptr, n, bank2, bank1, slab2, slab1, CUR(c), ev);
              else launch_resblock_bwd_full32_bf16(s, dy, a_fwd, x_fwd, dx, nullptr, n, bank2, bank1, slab2, slab1, CUR(c)); }
            push_slab(c, i2, grid); push_slab(c, i1, grid);
            ev_taken = c16 && ev != nullptr;
        } else {
            // both data gradients of a residual block in one launch (resblock_bf16.hip): the gradient of conv1's output goes
            // to HBM once (the weight-gradient kernels read it) and to LDS for the second transposed conv.  History of this fallback, from
            // before the whole-backward kernels above took the three residual shapes: against two dgrad launches the fused data
            // gradients measured 14.5 vs 15.9 ms per iteration at 16 channels @32x32, equal at 32 @8x8, and lost at 32 @16x16 (10.2 vs 8.3 ms)
            { ProfScope ps(c, PC_RESBLOCK_BWD + (int)s, n, px * ch * 2.0 * 5, 2.0 * px * 18.0 * ch * ch);
              launch_resblock_bwd_bf16(s, dy, a_fwd, x_fwd, Ga, dx, n, bank2, bank1, CUR(c)); }
            conv_wgrad(c, l2, a_fwd, nullptr, 1, dy, n);
            conv_wgrad(c, l1, x_fwd, nullptr, 1, Ga, n);
        }
    };
    residual(b * 5 + 3, G, k.A2, k.P1, Gb, nullptr);      // res2: P2 = conv2(relu(A2)) + P1 ; A2 = conv1(relu(P1))
    residual(b * 5 + 1, Gb, k.A1, k.P0, G, done_ev);      // res1: P1 = conv2(relu(A1)) + P0 ; A1 = conv1(relu(P0))
    return ev_taken;
}
// block2.conv / block3.conv and their max pool, bf16: both consumers of the conv-output gradient rebuild it from (pooled gradient G,
// arg-max); the gradient of the block's input goes to Gin
static void backward_conv_pool_bf16(mi_ctx* c, int b, int n, const float* G, float* Gin) {
    const Block& k = c->blk[b];
    const int layer = b * 5;
    const ConvLayer& L = c->convs[layer];
    const int fgrid = conv_bwd_fused_grid(L.shape, n);
    if (fgrid > 0) {        // block2.conv: data AND weight gradient in one launch (the max-pool backward gather runs once)
        ConvArgs a{};
        a.in = G; a.pool_arg = k.PI; a.out = Gin; a.n = n; a.bf16 = 1; a.wbank = c->banks + L.bank_d;
        a.wg_in = c->blk[b - 1].P2; a.wg_partial = c->slabs + c->slab_off[layer];
        const double px = (double)n * L.hw * L.hw;
        { ProfScope ps(c, PC_CONV_DGRAD + (int)L.shape, n, 2.0 * (px / 4 * L.cout + 3.0 * px * L.cout + 2.0 * px * L.cin), 2.0 * px * 18.0 * L.cin * L.cout);      // 8(d): pool bwd p + 2X, conv bwd X + 2I
          launch_conv_dgrad(L.shape, a, CUR(c)); }
        push_slab(c, layer, fgrid);
    } else {
        conv_wgrad(c, L, c->blk[b - 1].P2, nullptr, 0, G, n, k.PI);
        conv_dgrad(c, L, G, nullptr, nullptr, Gin, n, k.PI);
    }
}

static const float* backward_impala_bf16(mi_ctx* c, const InputSrc& src, int n, const BwdOpts& o) {
    const bool fc16 = n >= 1024;
    const bool fork1 = fc16 && o.side != nullptr && !tl_stream;
    const bool fork2 = c->side_on && !tl_stream && n >= 1024 && c->slab_desc_cached_n == n;
    float *Gout = c->GP[0], *Ga = c->GP[1], *Gb = c->GP[2];
    // embedder.fc: weight / bias gradient (on the side stream when the pass has a job for it), then the data gradient
    if (fork1) fork_stats_and_fc(c, n, *o.side);
    else if (fc16) {
        fc_refresh(c);
        { const double H = c->H;
          ProfScope ps(c, PC_GEMM, n, 2.0 * n * 2048 + 4.0 * n * H + 4.0 * 2048 * H, 2.0 * n * 2048 * H);
          launch_fc_tn(c->dfeat, (const unsigned short*)c->blk[2].P2, c->grads + c->fc.w_off, c->gemm_ws, (size_t)8 << 20, c->H, 2048, n, CUR(c)); }
        launch_colsum_acc(c->dfeat, n, c->H, c->H, c->grads + c->fc.b_off, c->col_ws, CUR(c));
    } else
        linear_wgrad(c, c->dfeat, c->blk[2].P2, 1, c->grads + c->fc.w_off, c->grads + c->fc.b_off, n, 2048, c->H, 1);
    issue_grad_allreduce(c, c->fc.w_off, c->n_params - c->fc.w_off, false);       // region A: fc + heads gradients are final
    if (fc16) {
        const double H = c->H;
        ProfScope ps(c, PC_GEMM, n, 4.0 * n * H + 2.0 * 2048 * H + 2.0 * 2.0 * n * 2048, 2.0 * n * 2048 * H);
        launch_fc_dgrad_bf16(c->dfeat, c->fc_wt, c->blk[2].P2, Gout, n, c->H, CUR(c));
    } else
        linear_dgrad(c, c->dfeat, c->params + c->fc.w_off, c->blk[2].P2, Gout, n, 2048, c->H, 1);
    fs_gradient(c, n, Gout, o);
    // blocks 3 and 2: residual pair, then the block's conv + pool (its data gradient lands in Ga: swap)
    for (int b = 2; b >= 1; --b) {
        backward_residual_pair(c, b, n, Gout, Ga, Gb, nullptr);
        backward_conv_pool_bf16(c, b, n, Gout, Ga);
        std::swap(Gout, Ga);
    }
    // block 1: its res1 is the last launch in front of the second fork, so the fork event is that launch's own completion
    const bool fork2_on_launch = backward_residual_pair(c, 0, n, Gout, Ga, Gb, fork2 ? c->ev_side_fork : nullptr);
    const float* const first = Gout;          // the gradient of block 1's pooled map
    int slabs_done = 0;          // leading entries of the slab table already summed on the side stream
    if (fork2 && c->slab_desc_n >= 1) slabs_done = fork_slab_sums(c, fork2_on_launch);
    conv_wgrad(c, c->convs[0], nullptr, &src, 0, Gout, n, c->blk[0].PI);          // block1.conv, pool backward fused into the staging
    if (fork1 || slabs_done) hipStreamWaitEvent(c->stream, c->ev_side_join, 0);   // join: statistics, fc gradients (and the first slab sums) are in place behind this point
    conv_wgrad_reduce_all(c, n, slabs_done);
    issue_grad_allreduce(c, 0, c->fc.w_off, true);                                 // region B: the conv layers' gradients
    return first;
}

// backward from dY (n x (A+1)), or from dfeat (o.from_dfeat); gradients accumulate into c->grads.  Returns what backward_* return.
const float* net_backward(mi_ctx* c, const InputSrc& src, int n, const BwdOpts& o) {
    const bool impala = c->cfg.arch == MI_ARCH_IMPALA;
    // (value saliency of a recurrent policy and mi_minibatch_rec come in with d / d (embedder output) in c->dfeat already: no heads step)
    if (!o.from_dfeat) {
        const bool to_side = o.side != nullptr && !tl_stream;      // a side job: the side stream also sums the heads' slabs and forks on this launch's completion
        heads_backward(c, n, impala ? 1 : 0, c->H <= 256 && c->A + 1 <= 16 && !tl_ws, true, CUR(c), !to_side, to_side ? c->ev_side_fork : nullptr);
    }
    if (!impala) return backward_mlp(c, n);
    if (!c->bf) return backward_impala_fp32(c, src, n, o);
    return backward_impala_bf16(c, src, n, o);
}

// ------------------------------------------------------------------------------------------ estimates
int mi_compute_estimates(mi_ctx* c, float gamma, float lmbda, int32_t use_gae, int32_t normalize_adv) {
    ARG(c, "null"); JOIN(c);
    launch_gae(c->rew, c->done, c->value, c->adv, c->ret, c->T, c->E, gamma, lmbda, use_gae, c->stream);
    if (normalize_adv) {
        launch_advnorm_stats(c->adv, c->T * c->E, c->adv_stats, c->stream);
        launch_advnorm_apply(c->adv, c->T * c->E, c->adv_stats, c->stream);
    }
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}
int mi_adv_stats(mi_ctx* c, double s[3]) {
    ARG(c && s, "null"); JOIN(c);
    launch_advnorm_stats(c->adv, c->T * c->E, c->adv_stats, c->stream);
    HIPC(hipMemcpyAsync(s, c->adv_stats, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_adv_apply(mi_ctx* c, const double s[3]) {
    ARG(c && s, "null"); JOIN(c);
    HIPC(hipMemcpyAsync(c->adv_stats, s, 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    launch_advnorm_apply(c->adv, c->T * c->E, c->adv_stats, c->stream);
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}

// ------------------------------------------------------------------------------------------ minibatch / optimiser
static InputSrc minibatch_src(mi_ctx* c) {
    return InputSrc{obs_ring(c), c->d_idx, 0};
}
// The N gather indices of a pass: fill(h) writes them into the next slot of the pinned index ring (a slot is rewritten only after the
// pull that read it has completed), a kernel pulls them into d_idx.
// "slot read" marker: an event record between the pull and the first conv kernel is a ~5 us bubble on the main stream (kernel
// traces: 5-7 us between pull_i32 and repack_all); when the pass forks the side stream (deferred_slot set: the slot goes there, for
// SideJob::idx_slot), the marker is recorded THERE, behind the fork (which is behind the pull in main-stream order: fork_stats_and_fc)
template <typename Fill>
static int stage_indices(mi_ctx* c, int N, Fill fill, int* deferred_slot) {
    const int slot = c->idx_next;
    c->idx_next = (slot + 1) % mi_ctx::IDX_RING;
    if (c->idx_used[slot]) HIPC(hipEventSynchronize(c->idx_ev[slot]));     // the pull that read this slot is done
    int32_t* h = c->h_idx_ring[slot];
    fill(h);
    launch_pull_i32(h, c->d_idx, N, c->stream);              // (not hipMemcpyAsync: see pull_i32_kernel)
    if (deferred_slot) *deferred_slot = slot;
    else HIPC(hipEventRecord(c->idx_ev[slot], c->stream));
    c->idx_used[slot] = true;
    return 0;
}
// What every minibatch entry does behind its own refusals and before its first launch.  The refusals all share, worded behind the entry's
// prefix: the n_idx caller indices lie in [0, limit) (range_msg), no multirank pass is pending, the loss log has room for n_seg records.
// Then the pass's N gather indices (stage_indices; N == 0: an empty pass pulls nothing), the profiler's sampling decision, and rec_last.
template <typename Fill>
static int begin_pass(mi_ctx* c, const char* prefix, const int64_t* idx, int n_idx, int64_t limit, const char* range_msg, int n_seg, int N, Fill fill,
                      int* deferred_slot = nullptr) {
    auto refuse = [&](const char* why) { return fail(-1, std::string(prefix) + why); };
    for (int k = 0; k < n_idx; ++k) if (!(idx[k] >= 0 && idx[k] < limit)) return refuse(range_msg);
    if (!(c->pending_n < 0)) return refuse("previous multirank minibatch not finished");
    if (!(c->log_count + n_seg <= c->log_cap)) return refuse("loss log full: call mi_loss_log_read(reset=1)");
    if (N > 0) if (int r = stage_indices(c, N, fill, deferred_slot)) return r;
    c->prof.phase = 1;
    c->prof.sample_now = (c->prof.mb_count++ % c->prof.period) == 0;
    c->rec_last = false;
    return 0;
}
static const char kArgPrefix[] = "invalid argument: ";      // ARG's
static auto copy_indices(const int64_t* idx, int n) { return [=](int32_t* h) { for (int k = 0; k < n; ++k) h[k] = (int32_t)idx[k]; }; }
// Where record log_count goes: its row of the statistics ring, its rank-local feature-sparsity value, its loss-log record
struct LogSlot { float *ring, *fsr, *log; };
static LogSlot log_slot(const mi_ctx* c) { return {c->stats_ring + (size_t)c->log_count * 32, c->fs_ring + c->log_count, c->loss_log + (size_t)c->log_count * 8}; }
static SegTab seg_tab(const int32_t* seg_n, int n_seg) {
    SegTab st{};
    st.n_seg = n_seg;
    for (int k = 0; k < n_seg; ++k) st.start[k + 1] = st.start[k] + seg_n[k];
    return st;
}
static LossArgs loss_args(mi_ctx* c, int n, int n_global, const mi_hparams* hp) {
    LossArgs a{};
    a.hout = c->hout; a.idx = c->d_idx; a.act = c->act; a.old_logp = c->logp; a.old_value = c->value; a.ret = c->ret; a.adv = c->adv;
    a.dY = c->dY; a.partial = c->loss_partial; a.stats = c->loss_stats; a.n = n; a.A = c->A;
    a.inv_n_global = 1.0f / (float)n_global;
    a.value_from_logits = c->lse;
    a.hp = LossHP{hp->eps_clip, hp->value_coef, hp->entropy_coef, hp->x_entropy_coef, hp->entropy_multiplier, hp->fs_coef};
    return a;
}
// loss terms + logged statistics of all segments on the main stream, one launch each (the pass that forks the side stream runs the
// metric and the records there instead: fork_stats_and_fc); with_dY: the sample gradients come out of the same pass
static void loss_and_records(mi_ctx* c, const LossArgs& a, const SegTab& st, bool with_dY, int mode, float* ring, float* fsr, float* log) {
    const bool impala = c->cfg.arch == MI_ARCH_IMPALA;
    if (impala) launch_fs_metric_seg(c->blk[2].P2, c->bf, st, 2048, c->fs_scratch, c->fs_parts, c->stream);
    launch_loss_fwd_seg(a, st, with_dY, c->stream);
    launch_loss_finalize_seg(a, st, mode, ring, impala ? c->fs_parts : nullptr, 2048, fsr, log, c->stream);
}

// One forward + backward pass over n gathered samples that belong to n_seg GLOBAL minibatches (segment k = seg_n[k] consecutive
// entries of idx, every segment a global minibatch of n_global samples): per-sample gradients scale with 1 / n_global, the loss
// statistics are taken and logged per segment.  n_seg > 1 is gradient accumulation done in one launch set (agents/ppo.py:170-177
// sums the gradients of the accumulated minibatches before the optimizer step, so only the fp32 summation order changes); it
// needs a loss without batch-level terms (x_entropy_coef == 0, fs_coef == 0).
static bool side_eligible(const mi_ctx* c, int n, bool batch_terms) {
    return c->side_on && c->cfg.arch == MI_ARCH_IMPALA && c->bf && n >= 1024 && !batch_terms && !c->ar_armed && !c->comm && c->H <= 256 && c->A + 1 <= 16;
}
static int minibatch_impl(mi_ctx* c, const int64_t* idx, int32_t n, const int32_t* seg_n, int32_t n_seg, int32_t n_global, const mi_hparams* hp) {
    ARG(c && hp, "null"); JOIN(c); ARG(n >= 0 && n <= c->NB, "n_idx must be in [0, max_batch]"); ARG(n_global >= 1, "n_global");
    ARG(n == 0 || idx, "idx"); ARG(n_seg >= 1 && n_seg <= MI_MAX_SEG && seg_n, "1 .. 16 segments");
    { long long tot = 0; for (int k = 0; k < n_seg; ++k) { ARG(seg_n[k] >= 0, "negative segment"); tot += seg_n[k]; } ARG(tot == n, "segments do not add up to n_idx"); }
    const bool batch_terms = hp->x_entropy_coef != 0.f || hp->fs_coef != 0.f;
    ARG(hp->fs_coef == 0.f || c->multirank != 2, "fs_coef != 0 needs the column maxima over the GLOBAL minibatch before the backward pass: multirank mode 1");
    ARG(hp->fs_coef == 0.f || c->multirank == 0 || c->cfg.arch != MI_ARCH_IMPALA || c->gpos_n == n,
        "fs_coef != 0 on several ranks: call mi_minibatch_positions with this pass's global minibatch positions first");
    ARG(n_seg == 1 || (!batch_terms && c->multirank != 1), "several minibatches per call need x_entropy_coef == 0, fs_coef == 0 and multirank mode 0 or 2");
    // no batch-level loss terms, bf16 IMPALA at update size, gradients exchanged (if at all) behind the pass: metric + records leave the
    // critical path (net_backward forks); the in-library armed exchange hands region A over in the middle of the pass and keeps the old order
    const bool fork = side_eligible(c, n, batch_terms) && c->multirank != 1;
    SideJob side{};
    if (int r = begin_pass(c, kArgPrefix, idx, n, (int64_t)c->T * c->E, "minibatch index out of range", n_seg, n, copy_indices(idx, n), fork ? &side.idx_slot : nullptr)) return r;
    InputSrc src = minibatch_src(c);
    net_forward(c, src, n, {.train = true});
    const bool impala = c->cfg.arch == MI_ARCH_IMPALA;
    LossArgs a = loss_args(c, n, n_global, hp);
    if (c->multirank == 2)
        // deferred statistics: nothing in the backward pass needs the cross-rank sums when x_entropy_coef == 0 and fs_coef == 0, so this
        // rank's partial sums go to ring slot log_count and are summed over the ranks ONCE per optimize() (mi_loss_log_finalize)
        ARG(!batch_terms, "multirank mode 2 needs x_entropy_coef == 0 and fs_coef == 0 (use mode 1)");
    if (c->multirank != 1) {
        // modes 0 and 2: loss terms + logged statistics of all segments with one launch each.  The rank-local sums land in the
        // statistics ring (mode 0 derives the records right away, mode 2 after the cross-rank sum in mi_loss_log_finalize); without
        // batch-level terms the sample gradients dY come out of the same pass.
        const SegTab st = seg_tab(seg_n, n_seg);
        const LogSlot s = log_slot(c);
        a.stats = s.ring;                                // (x-entropy gradient, mode 0, n_seg == 1: the batch-mean action distribution)
        const int mode = c->multirank == 2 ? 1 : 3;
        float* log = c->multirank == 2 ? nullptr : s.log;
        if (fork) {
            launch_loss_fwd_seg(a, st, true, c->stream);
            side = SideJob{a, st, mode, s.ring, s.fsr, log, side.idx_slot};
        } else
            loss_and_records(c, a, st, !batch_terms, mode, s.ring, s.fsr, log);
        c->ring_args = a;
        c->log_count += n_seg;
        if (batch_terms) launch_loss_bwd(a, c->stream);
        BwdOpts o{.side = fork ? &side : nullptr};
        if (impala && hp->fs_coef != 0.f && n > 0) { o.fs_coef = hp->fs_coef; o.fs_groups = fs_groups_per_segment(n_seg); }
        net_backward(c, src, n, o);
        HIPC(hipGetLastError()); NETCHK(c);
        return 0;
    }
    // mode 1: the cross-rank sum of the statistics comes between the loss forward and backward (mi_minibatch_finish)
    if (impala) launch_fs_metric(c->blk[2].P2, c->bf, n, 2048, c->fs_scratch, c->fs_val, c->stream);
    c->fs_global_pending = impala && hp->fs_coef != 0.f;
    if (c->fs_global_pending) {      // this rank's per-column candidates; the caller max-all-reduces MI_PTR_FS_KEYS before mi_minibatch_finish
        if (n > 0) launch_fs_keys(c->blk[2].P2, c->bf, n, 2048, c->fs_scratch, fs_metric_groups(), c->d_gpos, c->fs_colmax, c->fs_arg, c->fs_keys, c->fs_keys_local, c->stream);
        else { HIPC(hipMemsetAsync(c->fs_keys, 0, 2048 * 8, c->stream)); HIPC(hipMemsetAsync(c->fs_keys_local, 0, 2048 * 8, c->stream)); }
    }
    c->gpos_n = -1;
    launch_loss_fwd(a, c->stream);
    launch_loss_finalize(a, loss_blocks(n), 1, nullptr, nullptr, c->stream);
    c->pending = a; c->pending_n = n;
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}

int mi_minibatch(mi_ctx* c, const int64_t* idx, int32_t n, int32_t n_global, const mi_hparams* hp) {
    return minibatch_impl(c, idx, n, &n, 1, n_global, hp);
}
int mi_minibatch_multi(mi_ctx* c, const int64_t* idx, int32_t n, const int32_t* seg_n, int32_t n_seg, int32_t n_global, const mi_hparams* hp) {
    return minibatch_impl(c, idx, n, seg_n, n_seg, n_global, hp);
}

// The same pass for an MLP context as two launches behind the index pull (mlp_fused.hip): mi_minibatch_multi's contract, opt-in.  Every
// refusal comes before any launch and before log_count, the index ring or the gradient buffer change.
static int fused_alloc(mi_ctx* c) {
    if (c->fu_terms) return 0;
    const size_t NB = c->NB;
    DevPool& m = c->pool; DevPool::Group all(m);
    for (size_t l = 0; l + 1 < c->mlp.size(); ++l) HIPC(m.dev(&c->fu_g[l], NB * c->mlp[l].out));
    HIPC(m.dev(&c->fu_terms, NB * 32));
    all.keep = true;
    return 0;
}
#define FUSED_ARG(cond, msg) do { if (!(cond)) return fail(-1, std::string("mi_minibatch_fused: ") + msg); } while (0)
int mi_minibatch_fused(mi_ctx* c, const int64_t* idx, int32_t n, const int32_t* seg_n, int32_t n_seg, int32_t n_global, const mi_hparams* hp) {
    FUSED_ARG(c && hp && idx && seg_n, "null argument"); JOIN(c);
    FUSED_ARG(c->cfg.arch == MI_ARCH_MLP, "the context's arch must be MI_ARCH_MLP (IMPALA contexts use mi_minibatch)");
    FUSED_ARG(!c->gru_on, "a recurrent context (mi_set_gru) is not supported");
    FUSED_ARG(c->multirank == 0, "multirank mode must be 0");
    FUSED_ARG(!c->ar_armed && !c->ar_inflight && !c->comm, "an armed or in-flight gradient exchange or an initialised communicator is not supported");
    FUSED_ARG(hp->x_entropy_coef == 0.f && hp->fs_coef == 0.f, "x_entropy_coef and fs_coef must be 0 (the batch-level terms need the two-phase loss of mi_minibatch)");
    { const std::string why = resident_shape_refusal(c); FUSED_ARG(why.empty(), why); }
    FUSED_ARG(c->cfg.obs_dim <= 16, "obs_dim must be at most 16");
    FUSED_ARG(n >= 1 && n <= c->NB, "n_idx must be in [1, max_batch]"); FUSED_ARG(n_global >= 1, "n_global must be at least 1");
    FUSED_ARG(n_seg >= 1 && n_seg <= MI_MAX_SEG, "1 .. 16 segments");
    { long long tot = 0; for (int k = 0; k < n_seg; ++k) { FUSED_ARG(seg_n[k] >= 1, "every segment needs at least one sample"); tot += seg_n[k]; } FUSED_ARG(tot == n, "segments do not add up to n_idx"); }
    if (int r = fused_alloc(c)) return r;
    if (int r = begin_pass(c, "mi_minibatch_fused: ", idx, n, (int64_t)c->T * c->E, "minibatch index out of range", n_seg, n, copy_indices(idx, n))) return r;
    const size_t L = c->mlp.size();
    FusedNet f = {};
    f.net = resident_net(c);
    for (size_t l = 0; l < L; ++l) { f.act[l] = c->mlp_act[l]; f.g[l] = l + 1 < L ? c->fu_g[l] : c->dfeat; }
    f.act[L] = c->feat;
    f.obs = c->obsf; f.obs_dim = c->cfg.obs_dim; f.dYh = c->dY; f.terms = c->fu_terms;
    LossArgs a = loss_args(c, n, n_global, hp);
    const LogSlot s = log_slot(c);
    a.stats = s.ring;
    launch_mlp_fused_pass(f, a, n, c->stream);
    launch_mlp_fused_reduce(f, a, seg_tab(seg_n, n_seg), n, c->grads, s.ring, s.log, c->stream);
    c->ring_args = a;
    c->log_count += n_seg;
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}

// Global minibatch positions of the NEXT mi_minibatch's rows (ascending; the rank's share of a global minibatch keeps the global order):
// needed when fs_coef != 0 on more than one rank -- ties between equal column maxima go to the row that comes first globally.
int mi_minibatch_positions(mi_ctx* c, const int32_t* gpos, int32_t n) {
    ARG(c && (gpos || n == 0), "null"); JOIN(c); ARG(c->cfg.arch == MI_ARCH_IMPALA && c->d_gpos, "IMPALA contexts only"); ARG(n >= 0 && n <= c->NB, "n");
    if (n > 0) {
        HIPC(hipStreamSynchronize(c->stream));                 // (the pinned staging buffer of the previous call is free; this path is not the fast one)
        memcpy(c->h_gpos, gpos, (size_t)n * 4);
        HIPC(hipMemcpyAsync(c->d_gpos, c->h_gpos, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    }
    c->gpos_n = n;
    return 0;
}
int mi_set_multirank(mi_ctx* c, int32_t enabled) { ARG(c, "null"); ARG(enabled >= 0 && enabled <= 2, "mode"); c->multirank = enabled; return 0; }

// multirank mode 2: after the caller summed stats_ring[0 .. log_count*32) over the ranks, derive every minibatch's log record
int mi_loss_log_finalize(mi_ctx* c) {
    ARG(c, "null"); JOIN(c); ARG(c->multirank == 2, "only in multirank mode 2");
    const bool impala = c->cfg.arch == MI_ARCH_IMPALA;
    launch_loss_finalize_records(c->ring_args, c->log_count, c->stats_ring, impala ? c->fs_ring : nullptr, c->loss_log, c->stream);
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}

int mi_minibatch_finish(mi_ctx* c) {
    ARG(c, "null"); JOIN(c); ARG(c->pending_n >= 0, "no pending minibatch");
    const bool impala = c->cfg.arch == MI_ARCH_IMPALA;
    if (c->fs_global_pending) launch_fs_from_keys(c->fs_keys, 2048, c->fs_val, c->stream);      // the metric of the GLOBAL minibatch (keys are all-reduced by now)
    launch_loss_finalize(c->pending, 0, 2, impala ? c->fs_val : nullptr, log_slot(c).log, c->stream);
    c->log_count++;
    launch_loss_bwd(c->pending, c->stream);
    InputSrc src = minibatch_src(c);
    BwdOpts o;
    if (c->fs_global_pending) { o.fs_coef = c->pending.hp.fs_coef; o.fs_from_keys = true; }
    net_backward(c, src, c->pending_n, o);
    c->fs_global_pending = false;
    c->pending_n = -1;
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}

// ------------------------------------------------------------------------------------------ IPL (algo: IPL)
// One minibatch of IPL.optimize (agents/IPL.py:125-192).  The loss reads the network at obs[t] AND obs[t + 1]; with one activation set the
// schedule is three forward and two backward passes:
//   1 forward(nobs), inference   -> nv = done ? rew : V(nobs)                      (ipl.hip next-value kernel)
//   2 forward(obs), training     -> loss kernel: pred, dY, g_next, the record      -> backward(obs)
//   3 forward(nobs), training    -> dY = {0 .., g_next}                            -> backward(nobs), into the same gradient buffer
// nobs = ring row idx + E (slot T holds the bootstrap observation).  Everything runs on the main stream (no pass has a side job).
static int ipl_alloc(mi_ctx* c) {
    if (c->ipl_idx2) return 0;
    const size_t NB = c->NB;
    DevPool& m = c->pool; DevPool::Group all(m);
    HIPC(m.dev(&c->ipl_idx2, NB)); HIPC(m.dev(&c->ipl_nv, NB)); HIPC(m.dev(&c->ipl_gnext, NB)); HIPC(m.dev(&c->ipl_pred, NB)); HIPC(m.dev(&c->ipl_rew, NB));
    HIPC(m.dev(&c->ipl_partial, (size_t)ipl_blocks(c->NB) * ipl_partial_cols(c->A)));
    all.keep = true;
    return 0;
}
int mi_ipl_minibatch(mi_ctx* c, const int64_t* idx, int32_t n, int32_t n_global, const mi_ipl_hparams* hp) {
    ARG(c && hp && idx, "null"); JOIN(c);
    ARG(c->multirank == 0, "mi_ipl_minibatch: multirank mode must be 0 (IPL runs on one rank)");
    ARG(!c->ar_armed && !c->ar_inflight, "mi_ipl_minibatch: an armed gradient exchange (mi_allreduce_arm) is not supported");
    ARG(!c->gru_on, "mi_ipl_minibatch: a recurrent context (mi_set_gru) is not supported");
    ARG(!c->lse, "mi_ipl_minibatch: value_from_logits is not supported");
    ARG(n <= c->NB, "mi_ipl_minibatch: n > max_batch");
    ARG(n >= 1, "mi_ipl_minibatch: n must be at least 1"); ARG(n_global >= 1, "n_global");
    if (int r = ipl_alloc(c)) return r;
    if (int r = begin_pass(c, kArgPrefix, idx, n, (int64_t)c->T * c->E, "minibatch index out of range", 1, n, copy_indices(idx, n))) return r;
    launch_ipl_shift_idx(c->d_idx, c->ipl_idx2, n, c->E, c->stream);
    const InputSrc obs = minibatch_src(c), nobs{obs_ring(c), c->ipl_idx2, 0};
    IplArgs a{};
    a.hout = c->hout; a.idx = c->d_idx; a.act = c->act; a.rew = c->rew; a.done = c->done;
    a.nv = c->ipl_nv; a.dY = c->dY; a.g_next = c->ipl_gnext; a.pred = c->ipl_pred; a.rew_out = c->ipl_rew; a.partial = c->ipl_partial;
    a.n = n; a.A = c->A; a.inv_n_global = 1.0f / (float)n_global;
    a.gamma = hp->gamma; a.alpha = hp->alpha; a.entropy_coef = hp->entropy_coef;
    a.entropy_modified = (hp->flags & MI_IPL_ENTROPY_MODIFIED) != 0; a.reward_incentive = (hp->flags & MI_IPL_REWARD_INCENTIVE) != 0;
    a.adv_incentive = (hp->flags & MI_IPL_ADV_INCENTIVE) != 0; a.zero_obs_seed = (hp->flags & MI_IPL_DEBUG_ZERO_OBS_SEED) != 0;
    net_forward(c, nobs, n, {});
    launch_ipl_next_value(a, c->hout, c->A + 1, c->A, c->stream);
    net_forward(c, obs, n, {.train = true});
    launch_ipl_loss(a, log_slot(c).log, c->stream);
    c->log_count += 1;
    c->ipl_last_n = n;
    net_backward(c, obs, n, {});
    net_forward(c, nobs, n, {.train = true});
    launch_ipl_next_seed(c->ipl_gnext, c->dY, n, c->A, c->stream);
    net_backward(c, nobs, n, {});
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}
int mi_ipl_read_pred(mi_ctx* c, float* pred_out, float* rew_out, int32_t n) {
    ARG(c && (pred_out || rew_out), "null"); JOIN(c);
    ARG(c->ipl_idx2 && c->ipl_last_n > 0, "mi_ipl_read_pred: no mi_ipl_minibatch has run"); ARG(n == c->ipl_last_n, "mi_ipl_read_pred: n != the last minibatch's size");
    if (pred_out) HIPC(hipMemcpyAsync(pred_out, c->ipl_pred, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (rew_out) HIPC(hipMemcpyAsync(rew_out, c->ipl_rew, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}

// clip + Adam + zero_grad with the caller's eps.  max_norm = +inf switches the clip off: adam_kernel's coef = min(max_norm / (norm + 1e-6), 1)
// is then inf > 1 -> exactly 1 for every finite norm, and g * 1 is g.
static int optimizer_step(mi_ctx* c, float lr, float max_norm, float eps, int32_t step, float* gnorm_out) {
    ARG(c, "null"); JOIN(c); ARG(step >= 1, "adam_step is 1-based");
    const AdamScalars a = adam_scalars(lr, step, eps);
    if (c->ar_inflight) { HIPC(hipStreamWaitEvent(c->stream, c->ev_ar_done, 0)); c->ar_inflight = false; }
    c->ar_issued = false; c->ar_armed = false;
    if (c->gru_train) {
        // clip_grad_norm_(policy.parameters()) with the GRU among the parameters (agents/ppo_pure.py:160): ONE norm over the flat and the GRU
        // gradients -- 128 partial sums each, every Adam launch adds up all 256 -- and one coefficient for both; same Adam, both zeroed
        const GruTensors g = gru_tensors(c);
        launch_sumsq_partials(c->grads, c->n_params, c->gru_sumsq, c->stream);
        launch_sumsq_partials(c->gru_g, (long long)gru_count(c), c->gru_sumsq + 128, c->stream);
        launch_adam(c->params, c->grads, c->adam_m, c->adam_v, c->n_params, c->gru_sumsq, 256, max_norm, lr, a.beta1, a.beta2, a.eps,
                    a.step_size, a.bc2_sqrt, c->gnorm, c->stream);
        for (int k = 0; k < 4; ++k)
            launch_adam(g.t[k].p, c->gru_g + g.t[k].off, c->gru_m + g.t[k].off, c->gru_v + g.t[k].off, (long long)g.t[k].len, c->gru_sumsq, 256, max_norm, lr, a.beta1,
                        a.beta2, a.eps, a.step_size, a.bc2_sqrt, nullptr, c->stream);
    } else {
        launch_sumsq_partials(c->grads, c->n_params, c->sumsq + 2, c->stream);          // 128 partial sums; the Adam kernel's waves add them up themselves
        launch_adam(c->params, c->grads, c->adam_m, c->adam_v, c->n_params, c->sumsq + 2, 128, max_norm, lr, a.beta1, a.beta2, a.eps,
                    a.step_size, a.bc2_sqrt, c->gnorm, c->stream);
    }
    c->fc_packed_valid = false;
    HIPC(hipGetLastError()); NETCHK(c);
    if (gnorm_out) {
        HIPC(hipMemcpyAsync(c->h_f, c->gnorm, 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        *gnorm_out = c->h_f[0];
    }
    return 0;
}
int mi_optimizer_step(mi_ctx* c, float lr, float max_norm, int32_t step, float* gnorm_out) {
    return optimizer_step(c, lr, max_norm, 1e-5f, step, gnorm_out);
}
int mi_optimizer_step_eps(mi_ctx* c, float lr, float max_norm, float eps, int32_t step, float* gnorm_out) {
    ARG(eps >= 0.f, "mi_optimizer_step_eps: eps must not be negative (or NaN)");
    ARG(max_norm > 0.f, "mi_optimizer_step_eps: max_grad_norm must be positive (+inf: no clipping)");
    return optimizer_step(c, lr, max_norm, eps, step, gnorm_out);
}

// ------------------------------------------------------------------------------------------ policy distillation (distill.py)
// The reference's distill.py:164-204 on the device: a teacher context labels every observation row of a data context's ring with its
// normalised log-probabilities (mi_distill_label), the student is fitted to them with MSELoss (mi_distill_minibatch: forward, loss
// kernels of distill.hip, backward; mi_optimizer_step_eps is its Adam) and scored forward-only (mi_distill_loss).
#define DST_ARG(entry, cond, msg) do { if (!(cond)) return fail(-1, std::string(entry ": ") + msg); } while (0)
// what both sides of a distillation call must be: non-recurrent, on one rank, with no gradient exchange armed
#define DST_SIDE(entry, c, who)                                                                                          \
    do {                                                                                                                 \
        DST_ARG(entry, !(c)->gru_on, "a recurrent context (mi_set_gru) is not supported (" who ")");                     \
        DST_ARG(entry, (c)->multirank == 0, "multirank mode must be 0 (" who "): distillation runs on one rank");        \
        DST_ARG(entry, !(c)->ar_armed && !(c)->ar_inflight, "an armed gradient exchange (mi_allreduce_arm) is not supported (" who ")"); \
    } while (0)
// the two contexts of a call read the same kind of observation rows and name the same actions, on one device
#define DST_PAIR(entry, a, b, who_b)                                                                                     \
    do {                                                                                                                 \
        DST_ARG(entry, ((a)->frames != nullptr) == ((b)->frames != nullptr), "the " who_b " reads another kind of observation (frames / rows) than the data context holds"); \
        DST_ARG(entry, (a)->obs_bytes_per_env == (b)->obs_bytes_per_env, "obs_dim of the " who_b " differs from the data context's"); \
        DST_ARG(entry, (a)->A == (b)->A, "n_actions of the " who_b " differs from the data context's");                   \
        DST_ARG(entry, (a)->cfg.device == (b)->cfg.device, "the " who_b " lives on another device than the data context"); \
    } while (0)
static int distill_alloc(mi_ctx* c, bool target) {
    DevPool& m = c->pool; DevPool::Group all(m);
    if (target && !c->dst_target) HIPC(m.dev(&c->dst_target, (size_t)c->T * c->E * c->A));
    if (!target && !c->dst_partial) { HIPC(m.dev(&c->dst_partial, (size_t)distill_blocks(c->NB))); HIPC(m.dev(&c->dst_acc, 1)); }
    all.keep = true;
    return 0;
}
// b's stream waits for what a's stream holds now (the events go back to the runtime on every return path, as in mi_copy_params)
static int order_behind(mi_ctx* a, mi_ctx* b) {
    if (a->stream == b->stream) return 0;
    hipEvent_t ev = nullptr;
    DevPool evs(hip_pool());
    HIPC(evs.event(&ev, hipEventDisableTiming));
    HIPC(hipEventRecord(ev, a->stream));
    HIPC(hipStreamWaitEvent(b->stream, ev, 0));
    return 0;
}
int mi_distill_label(mi_ctx* data, mi_ctx* teacher) {
    DST_ARG("mi_distill_label", data && teacher, "null context"); JOIN(data); JOIN(teacher);
    DST_SIDE("mi_distill_label", data, "data"); DST_SIDE("mi_distill_label", teacher, "teacher");
    DST_PAIR("mi_distill_label", data, teacher, "teacher");
    if (int r = distill_alloc(data, true)) return r;
    if (int r = order_behind(data, teacher)) return r;          // the rollout that filled data's ring
    const int rows = data->T * data->E;
    for (int r0 = 0; r0 < rows; r0 += teacher->NB) {
        const int n = std::min(teacher->NB, rows - r0);
        net_forward(teacher, InputSrc{obs_ring(data), nullptr, (long long)r0}, n, {});
        // the rows mi_forward hands out (same launcher, same arguments), written at their place in the ring instead of d_lp
        launch_logp_all(teacher->hout, n, teacher->A, data->dst_target + (size_t)r0 * data->A, teacher->lse ? teacher->d_val : nullptr, teacher->stream, teacher->lse);
    }
    HIPC(hipGetLastError()); NETCHK(teacher);
    if (int r = order_behind(teacher, data)) return r;          // data's passes read the labels; its next rollout must not overtake the teacher's reads
    data->dst_labelled = true;
    return 0;
}
int mi_distill_targets(mi_ctx* data, float* out, int64_t n) {
    DST_ARG("mi_distill_targets", data && out, "null argument"); JOIN(data);
    DST_ARG("mi_distill_targets", data->dst_labelled, "no mi_distill_label has filled this context's target ring");
    DST_ARG("mi_distill_targets", n == (int64_t)data->T * data->E * data->A, "n != T * E * n_actions");
    HIPC(hipMemcpyAsync(out, data->dst_target, (size_t)n * 4, hipMemcpyDeviceToHost, data->stream));
    HIPC(hipStreamSynchronize(data->stream));
    return 0;
}
int mi_distill_minibatch(mi_ctx* c, const int64_t* idx, int32_t n, int32_t n_global) {
    DST_ARG("mi_distill_minibatch", c && idx, "null argument"); JOIN(c);
    DST_SIDE("mi_distill_minibatch", c, "student");
    DST_ARG("mi_distill_minibatch", !c->lse, "value_from_logits on the student is not supported");
    DST_ARG("mi_distill_minibatch", n <= c->NB, "n > max_batch");
    DST_ARG("mi_distill_minibatch", n >= 1, "n must be at least 1"); DST_ARG("mi_distill_minibatch", n_global >= 1, "n_global must be at least 1");
    DST_ARG("mi_distill_minibatch", c->dst_labelled, "no mi_distill_label has filled this context's target ring");
    if (int r = distill_alloc(c, false)) return r;
    if (int r = begin_pass(c, "mi_distill_minibatch: ", idx, n, (int64_t)c->T * c->E, "minibatch index out of range", 1, n, copy_indices(idx, n))) return r;
    const InputSrc src = minibatch_src(c);
    net_forward(c, src, n, {.train = true});
    DistillArgs a{c->hout, c->d_idx, c->dst_target, c->dY, c->dst_partial, n, c->A, (float)(1.0 / ((double)n_global * c->A))};
    launch_distill_loss(a, 1.0 / ((double)n_global * c->A), log_slot(c).log, nullptr, 0, c->stream);
    c->log_count += 1;
    net_backward(c, src, n, {});
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}
int mi_distill_loss(mi_ctx* c, mi_ctx* data, float* loss_out) {
    DST_ARG("mi_distill_loss", c && data && loss_out, "null argument"); JOIN(c); JOIN(data);
    DST_SIDE("mi_distill_loss", c, "student"); DST_SIDE("mi_distill_loss", data, "data");
    DST_ARG("mi_distill_loss", !c->lse, "value_from_logits on the student is not supported");
    DST_PAIR("mi_distill_loss", data, c, "student");
    DST_ARG("mi_distill_loss", data->dst_labelled, "no mi_distill_label has filled the data context's target ring");
    if (int r = distill_alloc(c, false)) return r;
    if (int r = order_behind(data, c)) return r;                // the labels (and the ring) are complete
    const int rows = data->T * data->E;
    for (int r0 = 0; r0 < rows; r0 += c->NB) {
        const int n = std::min(c->NB, rows - r0);
        net_forward(c, InputSrc{obs_ring(data), nullptr, (long long)r0}, n, {});
        DistillArgs a{c->hout, nullptr, data->dst_target + (size_t)r0 * data->A, nullptr, c->dst_partial, n, c->A, 0.f};
        launch_distill_loss(a, 0.0, nullptr, c->dst_acc, r0 == 0, c->stream);
    }
    HIPC(hipGetLastError()); NETCHK(c);
    double* h = (double*)c->h_f;
    HIPC(hipMemcpyAsync(h, c->dst_acc, 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));                       // (so data's next rollout cannot overtake the reads of its ring)
    *loss_out = (float)(h[0] / ((double)rows * c->A));
    return 0;
}


// ------------------------------------------------------------------------------------------ GRU training (algo: ppo-pure)
// PPOPure.optimize of a recurrent policy (agents/ppo_pure.py:98-176; the training branch of GRU.forward, common/model.py:226-277): the
// hidden state is recomputed over the whole trajectory of the minibatch's envs and the gradient runs back through time into the GRU's
// four tensors.  They live beside the flat vector: their gradients and Adam moments are one vector {w_ih, w_hh, b_ih, b_hh} of
// 2 * 3H^2 + 2 * 3H floats.  Single rank, fp32 GRU arithmetic in both precision modes.
int mi_gru_train(mi_ctx* c, int32_t enabled) {
    ARG(c, "null"); JOIN(c); ARG(c->gru_on, "no GRU set: call mi_set_gru first");
    ARG(!enabled || gru_seq_width_ok(c->H), "GRU training needs a width (out_dim) that is a multiple of 64 in [64, 512]");
    if (enabled && !c->gru_g) {
        const size_t G = (size_t)gru_count(c), NB = c->NB, H = c->H;
        DevPool& m = c->pool; DevPool::Group all(m);
        HIPC(m.dev(&c->gru_g, G)); HIPC(m.dev(&c->gru_m, G)); HIPC(m.dev(&c->gru_v, G)); HIPC(m.dev(&c->gru_sumsq, (size_t)256));
        HIPC(m.dev(&c->rec_x, NB * H)); HIPC(m.dev(&c->rec_gi, NB * 3 * H)); HIPC(m.dev(&c->rec_sv, NB * 4 * H));
        HIPC(m.dev(&c->rec_dgi, NB * 3 * H)); HIPC(m.dev(&c->rec_dgh, NB * 3 * H)); HIPC(m.dev(&c->rec_hm, NB * H));
        HIPC(m.dev(&c->rec_mask, NB)); HIPC(m.dev(&c->rec_h0, NB * H));
        all.keep = true;
    }
    HIPC(hipStreamSynchronize(c->stream));
    c->gru_train = enabled != 0;
    return 0;
}
int mi_get_gru(mi_ctx* c, float* w_ih, float* w_hh, float* b_ih, float* b_hh) {
    ARG(c && w_ih && w_hh && b_ih && b_hh, "null"); JOIN(c); ARG(c->gru_on, "no GRU set");
    const GruTensors g = gru_tensors(c);
    float* dst[4] = {w_ih, w_hh, b_ih, b_hh};
    for (int k = 0; k < 4; ++k) HIPC(hipMemcpyAsync(dst[k], g.t[k].p, g.t[k].len * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_get_gru_grads(mi_ctx* c, float* w_ih, float* w_hh, float* b_ih, float* b_hh) {
    ARG(c && w_ih && w_hh && b_ih && b_hh, "null"); JOIN(c); ARG(c->gru_g, "GRU training is off: call mi_gru_train first");
    const GruTensors g = gru_tensors(c);
    float* dst[4] = {w_ih, w_hh, b_ih, b_hh};
    for (int k = 0; k < 4; ++k) HIPC(hipMemcpyAsync(dst[k], c->gru_g + g.t[k].off, g.t[k].len * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_get_gru_adam_state(mi_ctx* c, float* m, float* v, int64_t n) {
    ARG(c && m && v, "null"); JOIN(c); ARG(c->gru_g, "GRU training is off: call mi_gru_train first"); ARG(n == gru_count(c), "n != 2 * 3H^2 + 2 * 3H");
    HIPC(hipMemcpyAsync(m, c->gru_m, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)); HIPC(hipMemcpyAsync(v, c->gru_v, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_set_gru_adam_state(mi_ctx* c, const float* m, const float* v, int64_t n) {
    ARG(c && m && v, "null"); JOIN(c); ARG(c->gru_g, "GRU training is off: call mi_gru_train first"); ARG(n == gru_count(c), "n != 2 * 3H^2 + 2 * 3H");
    HIPC(hipMemcpyAsync(c->gru_m, m, (size_t)n * 4, hipMemcpyHostToDevice, c->stream)); HIPC(hipMemcpyAsync(c->gru_v, v, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}

// One recurrent minibatch: the n_env envs of env_idx x all T steps, rows time-major (row t * n_env + i = step t of env env_idx[i], the order
// of Storage.fetch_train_generator(recurrent=True), common/storage.py:93-110).  Embedder forward on all rows, the GRU over the
// trajectories from h0 with the masks 1 - done[t, e] (the done stored WITH step t, agents/ppo_pure.py:124 -- the rollout masks with the done
// of step t - 1), heads on h_t, the loss kernels of mi_minibatch, then back: heads, GRU through time, embedder from dX.
int mi_minibatch_rec(mi_ctx* c, const int64_t* env_idx, int32_t n_env, const float* h0, int32_t n_global, const mi_hparams* hp) {
    ARG(c && hp && env_idx && h0, "null"); JOIN(c);
    ARG(c->gru_train, "GRU training is off: call mi_gru_train first");
    ARG(!c->lse, "value_from_logits with a trained GRU (recurrent ppo-pure) is not supported");
    ARG(hp->fs_coef == 0.f, "algo ppo-pure has no feature-sparsity term: fs_coef must be 0");
    ARG(c->multirank == 0 && !c->ar_armed && !c->comm, "GRU training runs on a single rank: multirank modes 1 / 2 and the in-library gradient exchange are refused");
    ARG(n_env >= 1 && n_global >= 1, "n_env / n_global");
    ARG((int64_t)n_env * c->T <= c->NB, "n_env * T must not exceed max_batch");
    const int T = c->T, E = c->E, H = c->H, n = n_env, N = n_env * T;
    if (int r = begin_pass(c, kArgPrefix, env_idx, n, E, "env index out of range", 1, N,
                           [&](int32_t* h) { for (int t = 0; t < T; ++t) for (int i = 0; i < n; ++i) h[t * n + i] = (int32_t)(t * E + env_idx[i]); })) return r;
    HIPC(hipMemcpyAsync(c->rec_h0, h0, (size_t)n * H * 4, hipMemcpyHostToDevice, c->stream));      // (pageable source: copied at call time)
    InputSrc src = minibatch_src(c);
    const bool impala = c->cfg.arch == MI_ARCH_IMPALA;
    net_forward(c, src, N, {.heads = false, .train = true});                                 // embedder only: feat = x
    // the sequence forward writes h_t over feat (the heads and their backward read it there); x is needed again for dW_ih and, for IMPALA,
    // as the ReLU mask of dX
    HIPC(hipMemcpyAsync(c->rec_x, c->feat, (size_t)N * H * 4, hipMemcpyDeviceToDevice, c->stream));
    launch_gru_seq_mask(c->done, c->d_idx, c->rec_mask, N, c->stream);          // m[t, i] = 1 - done[t, e_i]
    linear_fwd(c, c->rec_x, 0, c->gru_wih, c->gru_bih, c->rec_gi, N, H, 3 * H, 0);
    launch_gru_seq_fwd(c->rec_gi, c->rec_h0, c->rec_mask, c->gru_whh, c->gru_bhh, c->feat, c->rec_sv, T, n, H, c->stream);
    net_heads(c, N);
    LossArgs a = loss_args(c, N, n_global, hp);      // (value_from_logits is 0 and fs_coef == 0 here by the checks above; stats is set to the ring slot below)
    a.hp.fs_coef = 0.f;                              // (+0: the check above also lets -0 through)
    const bool batch_terms = hp->x_entropy_coef != 0.f;
    const LogSlot s = log_slot(c);
    a.stats = s.ring;
    loss_and_records(c, a, seg_tab(&N, 1), !batch_terms, 3, s.ring, s.fsr, s.log);
    c->ring_args = a;
    c->log_count += 1;
    if (batch_terms) launch_loss_bwd(a, c->stream);
    // heads backward on h_t: no ReLU mask here (for IMPALA the embedder's final ReLU sits under x, not under h_t)
    heads_backward(c, N, 0, H <= 256 && c->A + 1 <= 16, false, c->stream);
    launch_gru_seq_bwd(c->dfeat, c->feat, c->rec_h0, c->rec_mask, c->rec_sv, c->gru_whh, c->rec_dgi, c->rec_dgh, c->rec_hm, T, n, H, c->stream);
    const size_t W = (size_t)3 * H * H, B = (size_t)3 * H;
    linear_wgrad(c, c->rec_dgi, c->rec_x, 0, c->gru_g, c->gru_g + 2 * W, N, H, 3 * H);                    // dW_ih += dGI^T X ; db_ih += colsum dGI
    linear_wgrad(c, c->rec_dgh, c->rec_hm, 0, c->gru_g + W, c->gru_g + 2 * W + B, N, H, 3 * H);           // dW_hh += dGH^T HM ; db_hh += colsum dGH
    linear_dgrad(c, c->rec_dgi, c->gru_wih, impala ? c->rec_x : nullptr, c->dfeat, N, H, 3 * H);          // dX = dGI W_ih (* x > 0: the embedder's final ReLU)
    net_backward(c, src, N, {.from_dfeat = true});
    c->rec_last = true;
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}

int mi_loss_log_read(mi_ctx* c, float* out, int32_t max_records, int32_t* n_records, int32_t reset) {
    ARG(c && n_records, "null"); JOIN(c);
    const int n = c->log_count < max_records ? c->log_count : max_records;
    if (out && n > 0) {
        HIPC(hipMemcpyAsync(out, c->loss_log, (size_t)n * 8 * 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    *n_records = n;
    if (reset) c->log_count = 0;
    return 0;
}

// ------------------------------------------------------------------------------------------ collectives (RCCL over xGMI)
int mi_comm_unique_id(void* out, size_t bytes) {
    ARG(out && bytes >= sizeof(ncclUniqueId), "need a 128-byte buffer");
    ncclUniqueId id;
    NCCLC(ncclGetUniqueId(&id));
    memcpy(out, &id, sizeof id);
    return 0;
}
int mi_comm_init(mi_ctx* c, const void* id_bytes, size_t bytes, int32_t rank, int32_t world) {
    ARG(c && id_bytes && bytes >= sizeof(ncclUniqueId), "null / short id"); ARG(world >= 1 && rank >= 0 && rank < world, "rank / world");
    ARG(!c->comm, "communicator already initialised");
    JOIN(c);
    HIPC(hipSetDevice(c->cfg.device));
    ncclUniqueId id;
    memcpy(&id, id_bytes, sizeof id);
    struct Undo { mi_ctx* c; bool keep = false; ~Undo() { if (!keep) mi_comm_destroy(c); } } undo{c};      // a failure below releases what it got
    NCCLC(ncclCommInitRank(&c->comm, world, id, rank));
    // The gradient regions travel on a side stream while the main stream may issue its own collectives (loss statistics, feature-
    // sparsity keys, advantage statistics).  One communicator driven from two streams has no defined order between the two streams'
    // operations; each stream therefore owns a communicator.  Both are used in the same host order on every rank (the update schedule
    // is rank-uniform: mi355/dist.py update_plan), which is what RCCL needs of two communicators on one device.
    NCCLC(ncclCommSplit(c->comm, 0, rank, &c->comm_grad, nullptr));
    c->comm_world = world; c->comm_rank = rank;
    HIPC(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    HIPC(c->comm_pool.event(&c->ev_ar_ready, hipEventDisableTiming));
    HIPC(c->comm_pool.event(&c->ev_ar_done, hipEventDisableTiming));
    HIPC(c->comm_pool.dev(&c->adv_all, (size_t)3 * world + 4));
    undo.keep = true;
    return 0;
}
int mi_comm_destroy(mi_ctx* c) {      // (also of a communicator mi_comm_init got only halfway through)
    if (!c || !c->comm) return 0;
    if (c->comm_stream) hipStreamSynchronize(c->comm_stream);
    hipStreamSynchronize(c->stream);
    if (c->comm_grad) { ncclCommDestroy(c->comm_grad); c->comm_grad = nullptr; }
    ncclCommDestroy(c->comm); c->comm = nullptr;
    c->comm_pool.release_all();
    if (c->comm_stream) { hipStreamDestroy(c->comm_stream); c->comm_stream = nullptr; }
    c->comm_world = 1; c->comm_rank = 0;
    c->ar_armed = c->ar_issued = c->ar_inflight = false;
    return 0;
}
int mi_allreduce_arm(mi_ctx* c) {
    ARG(c, "null"); ARG(c->comm, "no communicator: call mi_comm_init first"); ARG(!c->ar_inflight, "a gradient all-reduce is already in flight");
    c->ar_armed = true;
    return 0;
}
int mi_allreduce_grads(mi_ctx* c) {
    ARG(c, "null"); ARG(c->comm, "no communicator: call mi_comm_init first"); JOIN(c);
    if (c->ar_issued) return 0;              // the armed backward pass already sent both regions
    c->ar_armed = true;
    issue_grad_allreduce(c, 0, c->n_params, true);
    NETCHK(c);
    return 0;
}
int mi_allreduce_buffer(mi_ctx* c, int32_t which, int64_t n) {
    ARG(c, "null"); ARG(c->comm, "no communicator: call mi_comm_init first"); JOIN(c);
    if (which == MI_PTR_FS_KEYS) {                             // max over the ranks of the per-column candidates
        ARG(c->fs_keys && n == 2048, "MI_PTR_FS_KEYS: the 2048 keys of an IMPALA context");
        NCCLC(ncclAllReduce(c->fs_keys, c->fs_keys, 2048, ncclInt64, ncclMax, c->comm, c->stream));
        return 0;
    }
    float* p = nullptr; int64_t cap = 0;
    switch (which) {
        case MI_PTR_LOSS_STATS: p = c->loss_stats; cap = 32; break;
        case MI_PTR_STATS_RING: p = c->stats_ring; cap = (int64_t)c->log_cap * 32; break;
        case MI_PTR_GRADS: p = c->grads; cap = c->n_params; break;
        default: return fail(-1, "mi_allreduce_buffer: unknown buffer id");
    }
    ARG(n >= 1 && n <= cap, "count");
    NCCLC(ncclAllReduce(p, p, (size_t)n, ncclFloat, ncclSum, c->comm, c->stream));
    return 0;
}
// Storage.compute_estimates' advantage normalisation over ALL ranks' envs (common/storage.py:78-79): local {count, mean, M2} in fp64,
// all-gather, Chan merge and the apply pass, all on the device (no host round trip)
int mi_adv_normalize_global(mi_ctx* c) {
    ARG(c, "null"); ARG(c->comm, "no communicator: call mi_comm_init first"); JOIN(c);
    launch_advnorm_stats(c->adv, c->T * c->E, c->adv_stats, c->stream);
    NCCLC(ncclAllGather(c->adv_stats, c->adv_all, 3, ncclDouble, c->comm, c->stream));
    launch_advnorm_merge(c->adv_all, c->comm_world, c->adv_stats, c->stream);
    launch_advnorm_apply(c->adv, c->T * c->E, c->adv_stats, c->stream);
    HIPC(hipGetLastError());
    return 0;
}

int mi_device_ptr(mi_ctx* c, int32_t which, void** ptr, int64_t* n) {
    ARG(c && ptr && n, "null"); JOIN(c);
    switch (which) {
        case MI_PTR_GRADS: *ptr = c->grads; *n = c->n_params; return 0;
        case MI_PTR_LOSS_STATS: *ptr = c->loss_stats; *n = 32; return 0;
        case MI_PTR_PARAMS: *ptr = c->params; *n = c->n_params; return 0;
        case MI_PTR_STATS_RING: *ptr = c->stats_ring; *n = (int64_t)c->log_cap * 32; return 0;
        case MI_PTR_FS_KEYS: ARG(c->fs_keys, "IMPALA contexts only"); *ptr = c->fs_keys; *n = 2048; return 0;      // 2048 int64 keys
        default: return fail(-1, "unknown pointer id");
    }
}

// bit 0: run rollout-sized bf16 inference passes on the separate block-2 / block-3 kernels instead of the fused launch (parity A/B)
int mi_debug_flags(mi_ctx* c, int32_t flags) { ARG(c, "null"); JOIN(c); c->rollout_tail = !(flags & 1); c->no_pull = (flags & 4) != 0; c->side_on = !(flags & 16); return 0; }
