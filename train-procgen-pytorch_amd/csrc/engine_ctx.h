// Internal header of the engine's translation units (engine.hip: context, network program, update entries; rollout.hip: rollout steps,
// env groups, staged and recurrent entries; engine_ops.hip: the op-level and debug entry points that only tests and micro-benchmarks
// call; env_device.hip: the device-resident envs and their mi_env_* entries; env_resident.hip: their one-launch rollout;
// env_evaluate.hip: their one-launch evaluation).  It holds what they share and nothing else: the context, the error plumbing, and the
// few functions of engine.hip and rollout.hip that another file calls.
#pragma once
#include "common.h"
#include "devpool.h"
#include "../../include/mi355ppo.h"
#include <rccl/rccl.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#pragma GCC visibility push(hidden)      // (the member functions of a template would be exported otherwise)
#include "group_worker.h"
#pragma GCC visibility pop

#pragma clang diagnostic ignored "-Wc++20-designator"      // FwdOpts and BwdOpts are filled by name at every call site
#define MI_INTERNAL __attribute__((visibility("hidden")))      // shared by the two files, not part of the library's ABI

MI_INTERNAL extern thread_local std::string g_err;
// A worker thread of the pipelined rollout issues one env group's pass on that group's stream with that group's slice of the split-K
// workspace: the network program reads both through these thread-local overrides (null on every other thread: the context's own).
// (__thread, not thread_local: a file other than the defining one reaches an extern thread_local through an init-function check, and for
// these three, which have none, that check is a hidden weak undefined symbol -- its address is not null once the library is loaded)
MI_INTERNAL extern __thread hipStream_t tl_stream;
MI_INTERNAL extern __thread float* tl_ws;
MI_INTERNAL extern __thread size_t tl_ws_floats;
#define CUR(c) (tl_stream ? tl_stream : (c)->stream)
static inline int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIPC(x)                                                                                          \
    do {                                                                                                 \
        hipError_t e_ = (hipError_t)(x);      /* (the pool's calls return the backend's code as an int) */ \
        if (e_ != hipSuccess)                                                                            \
            return fail(-2, std::string(#x) + ": " + hipGetErrorString(e_) + " @" + std::to_string(__LINE__)); \
    } while (0)
#define ARG(c, msg) do { if (!(c)) return fail(-1, std::string("invalid argument: ") + msg); } while (0)
#define NETCHK(c) do { if (const char* lf_ = mi_launch_failed_take()) return fail(-4, lf_);                                   \
                       std::string m_ = net_err_take(c); if (!m_.empty()) return fail(-4, m_); } while (0)
// every entry point that issues work on the context's main stream first orders it behind the env-group streams of a pipelined rollout
#define JOIN(c) do { if ((c)->groups_live) { int r_ = join_groups(c); if (r_) return r_; } } while (0)


enum TKind { K_PLAIN = 0, K_CONVW, K_FCW };
struct TensorDesc {
    std::string name;
    int64_t ref_off, dev_off, n;
    int kind, co, ci;
};

struct ConvLayer { ConvShape shape; int64_t w_off, b_off; int cin, cout, hw; long long bank_f = -1, bank_d = -1; };   // bank offsets (bf16 mode) or -1
struct Block { float *C = nullptr, *P0 = nullptr, *A1 = nullptr, *P1 = nullptr, *A2 = nullptr, *P2 = nullptr; uint8_t* PI = nullptr; int cin = 0, cout = 0, hin = 0; };   // activation buffers hold fp32 or bf16 (ctx.bf)
struct Linear { int64_t w_off, b_off; int in, out; };

// ---- live kernel timing (bench.py roofline leg)
enum ProfClass { PC_CONV_FWD = 0, PC_CONV_DGRAD = 5, PC_CONV_WGRAD = 10, PC_POOL_FWD = 15, PC_POOL_BWD, PC_GEMM, PC_SLAB_REDUCE, PC_RESBLOCK, PC_RESBLOCK_BWD = PC_RESBLOCK + 5, PC_COUNT = PC_RESBLOCK_BWD + 5 };
struct ProfPending { hipEvent_t a, b; int cls, phase; long long units; double bytes, flops; };
struct Profiler {
    bool on = false;
    bool all_phases = false;       // false: update phase only (the rollout's ~5.6k tiny launches per iteration are not bracketed)
    int phase = 0;
    int period = 1, mb_count = 0;  // update phase: bracket every period-th minibatch (two event records per launch cost ~7 us of
    bool sample_now = true;        // stream time: 11 ms per hard-500 iteration when every launch is bracketed)
    std::vector<ProfPending> pend;
    std::vector<hipEvent_t> pool;      // idle events
    std::deque<hipEvent_t> made;       // every event made so far (owned by the context's pool, like all its events)
    double ms[2][PC_COUNT] = {};
    long long launches[2][PC_COUNT] = {}, units[2][PC_COUNT] = {};
    double bytes[2][PC_COUNT] = {}, flops[2][PC_COUNT] = {};
};

// ---- the device-resident env of a context (env_device.hip: mi_env_*_create fills it, every other mi_env_* entry reads it)
struct CartPoleArgs { double low[9], high[9], x_threshold, theta_threshold; int max_steps; };      // kernel arguments of the envs
struct CartPoleSwingArgs { double low[9], high[9], x_threshold; int max_steps; };
struct MountainCarArgs { double low[5], high[5], left_boundary, max_speed, force, goal_velocity; int max_steps, sparse_rewards; };
struct DeviceEnv;
// What the resident rollout kernel (env_resident.hip) reads of the network and writes of the rings.  RES_R envs per workgroup (one MFMA
// M tile, a compile-time choice); an MLP of at most RES_MAX_LAYERS layers, each at most RES_MAX_WIDTH wide (the LDS activation rows).
// vec[l] / heads_vec: the layer's weight rows may be loaded 16 bytes at a time (in a multiple of 16 and w_off a multiple of 4).
#define RES_R 16
#define RES_MAX_LAYERS 16
#define RES_MAX_WIDTH 512
struct ResidentNet {
    const float* params;
    int n_layers, H, lse, heads_vec;
    int in[RES_MAX_LAYERS], out[RES_MAX_LAYERS], vec[RES_MAX_LAYERS];
    long long w_off[RES_MAX_LAYERS], b_off[RES_MAX_LAYERS], wh_off, bh_off;
};
struct ResidentRings { float* obs; int32_t* act; float *logp, *value, *rew, *done; };
// What the evaluation kernel (env_evaluate.hip, mi_env_evaluate) reads and writes beside the network: the planted episode starts
// [E][K][W] (null: every episode starts from the reset stream) and one record per env and episode, [E][K] each, start [E][K][W].
struct EvalRecords { const double* starts; double* ret; int32_t *length, *terminated; float* value0; double* start; };
// What the fused MLP minibatch pass (mlp_fused.hip, mi_minibatch_fused) reads and leaves behind for its second launch: the network as
// the resident rollout sees it (same limits), the observation ring, and per-row buffers of max_batch rows -- act[l] the input of layer
// l (act[0]: the gathered observations, act[n_layers]: the embedder output), g[l] the gradient of layer l's output, dYh the heads'
// gradient [n][A + 1], terms the per-sample loss terms [n][32].
struct FusedNet {
    ResidentNet net;
    const float* obs; int obs_dim;
    float* act[RES_MAX_LAYERS + 1];
    float* g[RES_MAX_LAYERS];
    float *dYh, *terms;
};
void launch_mlp_fused_pass(const FusedNet& f, const LossArgs& a, int n, hipStream_t st);
// segment k's statistics row stats_base + 32 k and record log_base + 8 k; grads += the pass's gradient
void launch_mlp_fused_reduce(const FusedNet& f, const LossArgs& a, const SegTab& seg, int n, float* grads, float* stats_base, float* log_base,
                             hipStream_t st);
// One constant row per env: how the messages of its create call name it, its state width (= observation width) and action count, what
// mi_env_step answers to an action out of range, and the launchers of its step, reset, resident rollout and evaluation kernels.
struct EnvOps {
    const char *entry, *columns, *actions, *action_range;
    int width, n_actions;
    // one step of all E envs on act[E]: advances state / n_steps / episode, writes the next observation (E x width), reward and done (E)
    void (*step)(const DeviceEnv& d, int E, const int32_t* act, float* obs_next, float* rew, float* done, hipStream_t st);
    void (*reset)(const DeviceEnv& d, int E, float* obs, hipStream_t st);
    // a whole rollout in one launch (mi_env_rollout_resident): what T + 1 policy steps and T env steps leave in the rings and the env
    void (*rollout)(const DeviceEnv& d, const ResidentNet& net, const ResidentRings& ring, int E, int T, unsigned long long seed, hipStream_t st);
    // K whole episodes of every env in one launch (mi_env_evaluate): reads the env's arguments and seed only, writes the records only
    void (*evaluate)(const DeviceEnv& d, const ResidentNet& net, const EvalRecords& rec, int E, int K, long long first_episode,
                     unsigned long long seed, bool greedy, hipStream_t st);
    int (*max_steps)(const DeviceEnv& d);      // the create call's max_steps, as the env's Args member holds it
};
// ops: null = no env.  state [E][width] fp64, steps of the running episode, episode number; the staging slot of mi_env_step {actions,
// next observation, reward, done}, which leaves the rings alone.
struct DeviceEnv {
    const EnvOps* ops = nullptr;
    union { CartPoleArgs cp; CartPoleSwingArgs cs; MountainCarArgs mc; } args = {};
    unsigned long long seed = 0;
    double* state = nullptr; int32_t* nsteps = nullptr; long long* episode = nullptr;
    int32_t* s_act = nullptr; float *s_obs = nullptr, *s_rew = nullptr, *s_done = nullptr;
};

// ---- one env group of the pipelined rollout (rollout.hip).  GroupJob: one step of the group, as the submitting thread hands it to the
// group's worker (group_worker.h: one host thread per group issues that group's copies + launches; a step is ~9 API calls = ~30 us of
// host time).  stream: a lane borrowed from the process-wide registry (lanes.h, g_lanes in rollout.hip), never a stream of the
// context's own.  forked: the stream is ordered behind the main stream's work; dirty: it has work the main stream has not been ordered
// behind yet; busy / last / ticket: the step in flight; rec_ok: mi_rec_begin has run since the group last started a rollout (t == 0).
struct GroupJob { int t; const void* frames; size_t bytes; bool pull; bool have_rd, last; const float* u; unsigned long long seed; unsigned ticket; };
struct RolloutGroup {
    hipStream_t stream = nullptr; int prio = 0; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool forked = false, busy = false, last = false, dirty = false, rec_ok = false; unsigned ticket = 0;
    GroupWorker<GroupJob, mi_ctx>* worker = nullptr;
};
static constexpr int MAX_LANE_DEVICES = 64;      // one lane registry per device (rollout.hip)

MI_INTERNAL const DevPool::Backend* hip_pool();      // engine.hip: hipMalloc / hipHostMalloc / hipEventCreateWithFlags and their frees, counted
struct mi_ctx {
    Profiler prof;
    mi_config cfg = {};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int T = 0, E = 0, A = 0, H = 0, NB = 0;
    bool bf = false;      // IMPALA activations / activation gradients stored as bf16 (mi_config.precision == 1)
    double es = 4.0;      // bytes per activation element
    int64_t n_params = 0;
    std::vector<TensorDesc> tensors;
    float *params = nullptr, *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr;
    // rollout
    uint8_t* frames = nullptr;      // impala
    float* obsf = nullptr;          // mlp
    size_t obs_bytes_per_env = 0;
    float *rew = nullptr, *done = nullptr, *logp = nullptr, *adv = nullptr, *ret = nullptr, *value = nullptr;
    int32_t* act = nullptr;
    double* adv_stats = nullptr;
    // network
    std::vector<ConvLayer> convs;
    Block blk[3];
    Linear fc = {};          // impala fc 2048->H (output_dim)
    std::vector<Linear> mlp;
    std::vector<float*> mlp_act;   // X0 (input), h1..hL
    int64_t wh_off = 0, bh_off = 0;        // heads: (A+1) x H weights, (A+1) bias (device order)
    float *feat = nullptr, *hout = nullptr, *dY = nullptr, *dfeat = nullptr, *GC = nullptr, *GP[3] = {};
    int lse = 0; float* d_val = nullptr;                  // value_from_logits (common/policy.py:77-78); d_val: mi_forward's values [NB] in that mode
    float* slabs = nullptr; size_t slab_floats = 0;
    void* sal_dc = nullptr; float* sal_dx = nullptr;       // value saliency: conv-out gradient temp (bf16 mode), input gradient
    long long slab_off[15] = {}; SlabDesc h_slab_desc[15] = {}; SlabDesc* d_slab_desc = nullptr; int slab_desc_n = 0, slab_desc_cached_n = -1;   // per-layer slab regions; ONE reduce launch per backward pass
    float *gemm_ws = nullptr, *col_ws = nullptr, *fs_scratch = nullptr, *fs_val = nullptr; size_t gemm_ws_floats = 0;      // split-K / column-sum workspaces: per context
    float* lut = nullptr;
    unsigned short* lut16 = nullptr;     // uint8 -> bf16(k/255) table (bf16 mode, block1.conv)
    uint8_t* stage_frames = nullptr; float* stage_obs = nullptr;
    int32_t* d_idx = nullptr;
    float *loss_partial = nullptr, *loss_stats = nullptr, *loss_log = nullptr; int log_count = 0, log_cap = 4096;
    double* fs_parts = nullptr;                                     // [MI_MAX_SEG][8] column-block sums of the feature-sparsity metric
    float *stats_ring = nullptr, *fs_ring = nullptr; LossArgs ring_args = {};      // multirank mode 2: per-minibatch raw stats [log_cap][32] (+ rank-local fs), finalised after ONE all-reduce
    double* sumsq = nullptr; float* gnorm = nullptr;
    float* d_u = nullptr; float* d_lp = nullptr;
    unsigned short* banks = nullptr; BankDesc* d_bank_desc = nullptr; int n_banks = 0;   // bf16 mode: pre-packed conv filter banks
    unsigned short* c1_bank = nullptr;                                   // bf16 mode: block1.conv forward bank (conv1 kernels' LDS layout)
    unsigned short *fc_wp = nullptr, *fc_wt = nullptr;            // bf16 mode: packed fc.weight images ([H][2048] and [2048][H])
    bool fc_packed_valid = false;
    float *d_pack = nullptr, *h_pack = nullptr, *h_rd = nullptr, *d_rd = nullptr;     // packed rollout read-back {act,logp,value} x E ; packed {rew,done} upload
    unsigned *d_done_ctr = nullptr, *h_flag = nullptr, roll_ticket = 0;   // rollout step: workgroup counter, host-visible completion ticket (heads_sample_kernel)
    int32_t* s_act = nullptr; float *s_logp = nullptr, *s_val = nullptr; bool staged_valid = false;
    // recurrent rollout (GRU cell, never trained)
    bool gru_on = false; float *gru_wih = nullptr, *gru_whh = nullptr, *gru_bih = nullptr, *gru_bhh = nullptr, *h_state = nullptr, *h_masked = nullptr, *gru_gi = nullptr, *gru_gh = nullptr, *d_done = nullptr;
    float *gru_x = nullptr, *gru_dg = nullptr;      // value saliency through the GRU: the cell's input (embedder output, FwdOpts::keep_gru_x), d gates
    // pinned host staging
    // index staging ring: a slot is rewritten only after the H2D copy that read it has completed
    static constexpr int IDX_RING = 32;
    int32_t* h_idx_ring[IDX_RING] = {}; hipEvent_t idx_ev[IDX_RING] = {}; bool idx_used[IDX_RING] = {}; int idx_next = 0;
    float* h_f = nullptr; int32_t* h_i = nullptr; size_t h_f_floats = 0;
    int multirank = 0;
    LossArgs pending = {}; int pending_n = -1;
    // pipelined rollout (mi_rollout_submit / mi_rollout_wait): contiguous env groups, each on its own stream with its own rows of the
    // activation buffers, so that one group's frame upload + forward runs beside the host's wait for another group's actions
    static constexpr int MAX_GROUPS = 4;
    int n_groups = 1; hipStream_t main_stream = nullptr; RolloutGroup grp[MAX_GROUPS]; bool groups_live = false;
    std::atomic<int64_t> copy_slot_ns{0}; double copy_rate_bytes_per_us = 40000.0;      // uploads of the env groups take turns on the PCIe link (group_issue)
    std::unordered_map<const void*, bool> pull_ok; bool no_pull = false;      // frame buffers a kernel may read (mi_debug_flags bit 2: always DMA)
    // Side stream of a minibatch pass: the logged statistics (feature-sparsity metric, loss records) and embedder.fc's weight / bias
    // gradients are needed by nobody before the optimizer step, so they run beside the backward pass instead of in front of it
    // (seven small launches + fc_tn: ~65 us of kernels per 2.7 ms minibatch, of which the update gets ~15 us back -- 64.6 -> 64.2 ms per
    // iteration, same-box A/B by the debug flag: fc_tn and the column maxima are real work that now shares the machine with fc_dgrad).
    // Fork after heads_bwd, join in front of the slab sums.  What the fork runs comes in with the pass: BwdOpts::side.
    hipStream_t side_stream = nullptr; hipEvent_t ev_side_fork = nullptr, ev_side_join = nullptr;
    bool side_on = true;           // mi_debug_flags bit 4 clears it (A/B tests)
    bool rollout_tail = true;          // bf16 inference passes of <= 256 samples run blocks 2 + 3 as one launch (mi_debug_flags bit 0 clears it: A/B tests)
    float* fs_colmax = nullptr; int* fs_arg = nullptr;      // feature-sparsity gradient (BwdOpts::fs_coef != 0): column maxima / first arg-max rows of the minibatch
    // ... on more than one rank (multirank mode 1): per-column candidates for the max-all-reduce (MI_PTR_FS_KEYS), this rank's own copy, and
    // the global minibatch positions of the pending pass's rows (mi_minibatch_positions)
    long long *fs_keys = nullptr, *fs_keys_local = nullptr; int32_t *d_gpos = nullptr, *h_gpos = nullptr; int gpos_n = -1; bool fs_global_pending = false;
    // data-parallel collectives (RCCL over xGMI), SURVEY 8(e): one communicator per context, a side stream for the gradient all-reduce;
    // mi_comm_init / mi_comm_destroy may be repeated on one context, so what they allocate has a pool of its own
    ncclComm_t comm = nullptr, comm_grad = nullptr; int comm_world = 1, comm_rank = 0; hipStream_t comm_stream = nullptr; hipEvent_t ev_ar_ready = nullptr, ev_ar_done = nullptr;   // comm: main-stream collectives; comm_grad: the side stream's
    bool ar_armed = false, ar_issued = false, ar_inflight = false; double* adv_all = nullptr;
    std::string net_err; std::mutex net_err_mu;   // set by the (void) network program on an unsupported launch (any thread); every entry point reports it as -4
    // recurrent policies on the pipelined rollout (mi_rec_begin, group_issue): hidden ring [T+1][E][H] -- slot t = the input hidden state of step t (slot 0 from
    // mi_rec_begin, slot t+1 written by step t's fused cell); pinned staging of mi_rec_begin's upload {hidden [E][H], done [E]} and the event
    // that frees it (RolloutGroup::rec_ok: mi_rec_begin has run since the group last started a rollout)
    float *h_ring = nullptr, *h_rec_stage = nullptr; hipEvent_t ev_rec = nullptr;
    // GRU training (mi_gru_train, mi_minibatch_rec: algo ppo-pure): gradients and Adam moments of the four GRU tensors as ONE vector
    // {w_ih, w_hh, b_ih, b_hh} beside the flat ones, the partial sums of the global gradient norm (128 flat + 128 GRU), and the buffers of a
    // recurrent minibatch pass, max_batch rows each: the embedder output x (the sequence forward overwrites feat with h_t), gi, the saved
    // gates, dgi / dgh, the masked input states, the masks 1 - done and the minibatch's initial states
    bool gru_train = false, rec_last = false; float *gru_g = nullptr, *gru_m = nullptr, *gru_v = nullptr; double* gru_sumsq = nullptr;
    float *rec_x = nullptr, *rec_gi = nullptr, *rec_sv = nullptr, *rec_dgi = nullptr, *rec_dgh = nullptr, *rec_hm = nullptr, *rec_mask = nullptr, *rec_h0 = nullptr;
    // IPL (mi_ipl_minibatch; allocated by its first call, max_batch rows each): ring rows of obs[t + 1], next values, d loss / d nv, the last
    // minibatch's pred / reward, the loss kernel's fp64 block partials
    int32_t* ipl_idx2 = nullptr; float *ipl_nv = nullptr, *ipl_gnext = nullptr, *ipl_pred = nullptr, *ipl_rew = nullptr; double* ipl_partial = nullptr;
    int ipl_last_n = 0;
    // the fused MLP pass (mi_minibatch_fused; allocated by its first call, max_batch rows each): the output gradients of the layers below the
    // last (the last layer's is dfeat) and the per-sample loss terms
    float *fu_g[RES_MAX_LAYERS] = {}, *fu_terms = nullptr;
    // distillation (mi_distill_*; each allocated by the first call that needs it): the target ring [T * E][A] -- the teacher's normalised
    // log-probabilities of this context's observation rows, valid once a label call has filled it (dst_labelled) --, the loss kernel's
    // block partials (max_batch rows' worth) and the running fp64 sum of mi_distill_loss
    float* dst_target = nullptr; double *dst_partial = nullptr, *dst_acc = nullptr; bool dst_labelled = false;
    DeviceEnv env;                   // the device-resident env, if any (env_device.hip)
    struct mi_sae* sae = nullptr;     // the sparse-autoencoder agent's state (sae.hip: mi_sae_create; released by mi_sae_destroy or mi_destroy)
    // Every device buffer, pinned buffer and event above belongs to a pool (declared last: destroyed first, while the pointers it
    // nulls still exist).  ctx_release is the one place that lets go of them.
    DevPool pool{hip_pool()}, comm_pool{hip_pool()};
};

static inline char* obs_ring(mi_ctx* c) { return c->frames ? (char*)c->frames : (char*)c->obsf; }      // rollout observations [(T+1)][E]: uint8 frames or fp32 rows

// The MLP shapes the 16-row-tile kernels take (res_layer.h: the resident rollout and the fused minibatch pass have the same limits): the
// words of the first limit the context's network breaks, or "" -- the caller puts its entry's name in front.
static inline std::string resident_shape_refusal(const mi_ctx* c) {
    const size_t L = c->mlp.size();
    if (!(L >= 2 && L <= RES_MAX_LAYERS)) return "mlp_depth must be at least 2 and at most " + std::to_string(RES_MAX_LAYERS);
    if (!(c->cfg.mlp_width % 16 == 0 && c->cfg.mlp_width <= RES_MAX_WIDTH)) return "mlp_width must be a multiple of 16 and at most " + std::to_string(RES_MAX_WIDTH);
    if (!(c->H % 16 == 0 && c->H <= RES_MAX_WIDTH)) return "out_dim must be a multiple of 16 and at most " + std::to_string(RES_MAX_WIDTH);
    if (!(c->A + 1 <= 16)) return "n_actions must be at most 15";
    return "";
}
// the network of a context that passed resident_shape_refusal, as those kernels read it
static inline ResidentNet resident_net(const mi_ctx* c) {
    ResidentNet net = {};
    const size_t L = c->mlp.size();
    net.params = c->params; net.n_layers = (int)L; net.H = c->H; net.lse = c->lse;
    for (size_t l = 0; l < L; ++l) {
        const Linear& m = c->mlp[l];
        net.in[l] = m.in; net.out[l] = m.out; net.w_off[l] = m.w_off; net.b_off[l] = m.b_off;
        net.vec[l] = m.in % 16 == 0 && m.w_off % 4 == 0;
    }
    net.wh_off = c->wh_off; net.bh_off = c->bh_off; net.heads_vec = c->wh_off % 4 == 0;      // (H is a multiple of 16)
    return net;
}

// ------------------------------------------------------------------------------------------ engine.hip functions the op code calls
MI_INTERNAL std::string net_err_take(mi_ctx* c);                 // (the network program also runs on the env-group worker threads: guarded)
MI_INTERNAL void net_err_set(mi_ctx* c, const std::string& m);
MI_INTERNAL void sae_release(mi_ctx* c);                         // (defined in sae.hip; mi_destroy releases a live SAE through it)
MI_INTERNAL int join_groups(mi_ctx* c);                          // (defined in rollout.hip: JOIN)
MI_INTERNAL void to_device_layout(const TensorDesc& t, const float* ref, float* dev);
MI_INTERNAL void to_ref_layout(const TensorDesc& t, const float* dev, float* ref);
MI_INTERNAL std::vector<uint16_t> host_to_bf16(const float* x, size_t n);      // (defined in engine_ops.hip; mi_create builds the uint8 -> bf16 table with it)
// mi_debug_gru_seq issues the GEMMs of mi_minibatch_rec, mi_debug_step_latency the rollout step's forward pass: through the same functions
struct InputSrc { const void* base; const int32_t* idx; long long first; };   // frames or obs rows
// soff: first row of the activation buffers this pass may use (env groups of the pipelined rollout run side by side on
// their own streams, each in its own rows); 0 everywhere else.  keep_gru_x: the GRU cell's input survives in gru_x (value saliency)
struct FwdOpts { bool recurrent = false; bool heads = true; bool train = false; int soff = 0; bool keep_gru_x = false; };
MI_INTERNAL void net_forward(mi_ctx* c, const InputSrc& src, int n, const FwdOpts& o);
// What the side stream of a forking minibatch pass runs beside the backward pass (mi_ctx::side_stream): the records of the pass's segments
// (loss arguments, segment table, finalize mode, the log slot's three rows) and the "read" marker of index-ring slot idx_slot.
struct SideJob { LossArgs a; SegTab st; int mode; float* ring; float* fsr; float* log; int idx_slot = -1; };
// A backward pass (engine.hip net_backward); the defaults are the plain pass from dY.  from_dfeat: d / d (embedder output) is in dfeat
// already, no heads step.  fs_coef != 0: + fs_coef * d(feature sparsity) / d(block-3 output), over fs_groups row groups per segment, or
// (fs_from_keys) from the all-reduced keys of multirank mode 1.  side: the job of a pass that forks the side stream, on the caller's stack.
struct BwdOpts { bool from_dfeat = false; float fs_coef = 0.f; int fs_groups = 0; bool fs_from_keys = false; const SideJob* side = nullptr; };
// ---- engine.hip functions rollout.hip calls: the value saliency runs a whole backward pass (returns where it left the gradient of the
// first layer's output); a group's first step since the main stream last worked puts the packed bf16 filter images in place
MI_INTERNAL const float* net_backward(mi_ctx* c, const InputSrc& src, int n, const BwdOpts& o);
MI_INTERNAL void fc_refresh(mi_ctx* c);
static inline char* obs_stage(mi_ctx* c) { return c->stage_frames ? (char*)c->stage_frames : (char*)c->stage_obs; }   // staged observations [NB]
// the four GRU tensors {w_ih, w_hh, b_ih, b_hh}: device pointer, offset in the one vector of their gradients / Adam moments, length
struct GruTensor { float* p; size_t off, len; };
struct GruTensors { GruTensor t[4]; };
static inline GruTensors gru_tensors(mi_ctx* c) {
    const size_t H = c->H, W = 3 * H * H, B = 3 * H;
    return GruTensors{{{c->gru_wih, 0, W}, {c->gru_whh, W, W}, {c->gru_bih, 2 * W, B}, {c->gru_bhh, 2 * W + B, B}}};
}
// ---- rollout.hip functions other files call.  ctx_release: the groups' workers joined, then their streams synchronised; later, the
// lanes given back to the registry.  mi_env_rollout (env_device.hip) chains T + 1 policy steps with its env steps
MI_INTERNAL void rollout_groups_stop(mi_ctx* c);
MI_INTERNAL void rollout_lanes_return(mi_ctx* c);
MI_INTERNAL int issue_policy_step(mi_ctx* c, int32_t t, uint64_t seed, const float* du);
MI_INTERNAL void linear_fwd(mi_ctx* c, const float* X, int relu_x, const float* W, const float* b, float* Y, int n, int in, int out, int relu_out, int x_bf16 = 0);
MI_INTERNAL void linear_dgrad(mi_ctx* c, const float* dY, const float* W, const float* mask, float* dX, int n, int in, int out, int x_bf16 = 0);
MI_INTERNAL void linear_wgrad(mi_ctx* c, const float* dY, const float* X, int relu_x, float* gW, float* gb, int n, int in, int out, int x_bf16 = 0);

// The host scalars of one Adam step (lr, 1-based step): the one place they are computed, for mi_optimizer_step, mi_sae_optimizer_step and
// the op-level hook mi_op_adam alike.  beta1 / beta2 go to adam_kernel (which forms 1 - beta in fp32), w1 / w2 to sae_adam_kernel.
// eps: the agents' Adam(eps=1e-5) unless the caller says otherwise (mi_optimizer_step_eps: the distiller's torch default, 1e-8).
struct AdamScalars { float beta1, beta2, w1, w2, eps, step_size, bc2_sqrt; };
static inline AdamScalars adam_scalars(float lr, int step, float eps = 1e-5f) {
    const double b1 = 0.9, b2 = 0.999;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    return AdamScalars{(float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), eps, (float)((double)lr / bc1), (float)sqrt(bc2)};
}
