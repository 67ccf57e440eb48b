// The rollout side of the C ABI (include/mi355ppo.h): policy steps on the ring, the pipelined rollout over env groups, the staged
// entries (predict, value saliency, commit, forward) and the state of a recurrent rollout.  Host code only: every kernel it launches is
// declared in common.h, the network program it runs (net_forward, net_backward) is engine.hip's.
//
// One step of rows [e0, e0 + n) -- all E envs on the main stream (mi_rollout_step), or one env group on its lane -- is
//     [frames up] -> {rew, done} of step t-1 into the pinned hand-off rows -> forward -> [GRU cell] -> heads + sample
// and the last workgroup of the heads kernel publishes the step's ticket once the packed {act, logp, value} rows are visible to the
// host.  StepSlice names what such a step owns; the serial step and the group step share everything that is spelled in terms of it.
#include "engine_ctx.h"
#include "lanes.h"

// ------------------------------------------------------------------------------------------ what a step shares
// the caller's uniforms for rows [row0, row0 + rows), if given: *du = where the sampler reads them (null: it draws its own)
static int upload_u(mi_ctx* c, const float* u, hipStream_t st, int row0, int rows, const float** du) {
    *du = nullptr;
    if (u) { HIPC(hipMemcpyAsync(c->d_u + row0, u, (size_t)rows * 4, hipMemcpyHostToDevice, st)); *du = c->d_u + row0; }
    return 0;
}
// act / logp / value of the E envs to the caller through the pinned h_i / h_f, one stream wait: a field with a null device source is skipped,
// one with a null destination is copied to the host but not handed out; extra: one more copy to the caller in front of the wait
static int read_back_staged(mi_ctx* c, const int32_t* d_act, const float* d_logp, const float* d_val, int64_t* act_out, float* logp_out, float* value_out, void* extra_out = nullptr, const void* d_extra = nullptr, size_t extra_bytes = 0) {
    const size_t E = c->E;
    if (d_act) HIPC(hipMemcpyAsync(c->h_i, d_act, E * 4, hipMemcpyDeviceToHost, c->stream));
    if (d_logp) HIPC(hipMemcpyAsync(c->h_f, d_logp, E * 4, hipMemcpyDeviceToHost, c->stream));
    if (d_val) HIPC(hipMemcpyAsync(c->h_f + E, d_val, E * 4, hipMemcpyDeviceToHost, c->stream));
    if (extra_out) HIPC(hipMemcpyAsync(extra_out, d_extra, extra_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if (d_act && act_out) for (size_t e = 0; e < E; ++e) act_out[e] = c->h_i[e];
    if (d_logp && logp_out) memcpy(logp_out, c->h_f, E * 4);
    if (d_val && value_out) memcpy(value_out, c->h_f + E, E * 4);
    return 0;
}
// the packed {act, logp, value} x n a head kernel wrote to pinned memory, to the caller (the bootstrap step has no action / log-prob)
static inline void unpack_step(const float* pk, int n, bool last, int64_t* act_out, float* logp_out, float* value_out) {
    for (int e = 0; e < n; ++e) {
        if (act_out && !last) act_out[e] = (int64_t)pk[3 * e];
        if (logp_out && !last) logp_out[e] = pk[3 * e + 1];
        if (value_out) value_out[e] = pk[3 * e + 2];
    }
}
// The last workgroup of the head kernel publishes the ticket after all results (h_pack) are visible to the host and all reads of
// h_rd / u are done: spinning on it returns ~5 us earlier than hipStreamSynchronize (12.9 -> 8.1 us for launch + wait of a small
// kernel, scratch/synclat.hip), 257 times per iteration.  gone(), probed every 2^20 spins: the kernel can no longer publish (finished
// without a ticket, or failed); the caller then falls back to the stream wait, which reports the error.
template <typename Gone>
static inline bool wait_ticket(const volatile unsigned* flag, unsigned want, Gone gone) {
    for (unsigned long long spin = 0; spin < (1ull << 34); ++spin) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == want) return true;
        __builtin_ia32_pause();
        if ((spin & 0xfffff) == 0xfffff && gone()) break;
    }
    return false;
}

// What a rollout step of rows [e0, e0 + n) owns: the stream it runs on, its {rew[n], done[n]} hand-off rows and its packed result rows
// (pinned, device-visible), its workgroup counter and its ticket word.  g < 0: the serial step -- slot 0, all E rows, the main stream.
struct StepSlice { int e0, n; hipStream_t stream; float *h_rd, *h_pack; unsigned *ctr, *flag; };
static inline StepSlice step_slice(mi_ctx* c, int g) {
    if (g < 0) return StepSlice{0, c->E, c->stream, c->h_rd, c->h_pack, c->d_done_ctr, c->h_flag};
    const int n = c->E / c->n_groups, e0 = g * n;
    return StepSlice{e0, n, c->grp[g].stream, c->h_rd + 2 * e0, c->h_pack + 3 * e0, c->d_done_ctr + 1 + g, c->h_flag + 1 + g};
}
// {rew, done} of step t-1 come in with step t: pinned, device-visible staging -- the head kernel reads them straight from host memory
// and writes its packed result straight back, no copy kernels on the step's critical path (the ticket / the stream wait fences both)
static inline void stage_rew_done(const StepSlice& s, const float* rew_prev, const float* done_prev) {
    memcpy(s.h_rd, rew_prev, (size_t)s.n * 4); memcpy(s.h_rd + s.n, done_prev, (size_t)s.n * 4);
}
// ... and a GRU context masks its state with that done
static inline int done_to_gru(mi_ctx* c, const StepSlice& s) {
    HIPC(hipMemcpyAsync(c->d_done + s.e0, s.h_rd + s.n, (size_t)s.n * 4, hipMemcpyHostToDevice, s.stream));
    return 0;
}
// heads + sampler of the slice's rows on ring slot t (hin: what the heads read; du: upload_u's), {rew, done} into row t-1 of the ring
static inline void launch_step_heads(mi_ctx* c, const StepSlice& s, int t, const float* hin, const float* du, unsigned long long seed, bool have_rd, unsigned ticket) {
    const int E = c->E;
    const bool last = (t == c->T);
    const size_t o = (size_t)t * E + s.e0;
    launch_heads_sample(hin, c->params + c->wh_off, c->params + c->bh_off, s.n, c->H, c->A, du, seed, (unsigned long long)t * E + s.e0,
                        last ? nullptr : c->act + o, last ? nullptr : c->logp + o, c->value + o, s.h_pack, nullptr,
                        have_rd ? s.h_rd : nullptr, have_rd ? c->rew + o - E : nullptr, have_rd ? c->done + o - E : nullptr, s.stream,
                        s.ctr, s.flag, ticket, c->lse);
}

// ------------------------------------------------------------------------------------------ serial steps
// the launches of a policy step on ring slot t (forward, sample; du: the sampler's uniforms on the device or null), nothing else
int issue_policy_step(mi_ctx* c, int32_t t, uint64_t seed, const float* du) {
    const int E = c->E;
    InputSrc src{obs_ring(c), nullptr, (long long)t * E};
    c->prof.phase = 0;
    net_forward(c, src, E, {.recurrent = true});
    const bool last = (t == c->T);
    launch_sample(c->hout, E, c->A, du, seed, (unsigned long long)t * E, last ? nullptr : c->act + (size_t)t * E,
                  last ? nullptr : c->logp + (size_t)t * E, c->value + (size_t)t * E, c->stream, c->lse);
    HIPC(hipGetLastError()); NETCHK(c);
    return 0;
}
int mi_policy_step(mi_ctx* c, int32_t t, uint64_t seed, const float* u, int64_t* act_out, float* logp_out, float* value_out) {
    ARG(c, "null"); JOIN(c); ARG(t >= 0 && t <= c->T, "t out of range");
    const int E = c->E;
    const float* du;
    if (int r = upload_u(c, u, c->stream, 0, E, &du)) return r;
    if (int r = issue_policy_step(c, t, seed, du)) return r;
    const bool last = (t == c->T);
    if (!act_out && !logp_out && !value_out) { if (u) HIPC(hipStreamSynchronize(c->stream)); return 0; }
    const size_t o = (size_t)t * E;
    return read_back_staged(c, (act_out && !last) ? c->act + o : nullptr, (logp_out && !last) ? c->logp + o : nullptr, value_out ? c->value + o : nullptr, act_out, logp_out, value_out);
}

int mi_rollout_step(mi_ctx* c, int32_t t, const float* rew_prev, const float* done_prev, uint64_t seed, const float* u,
                    int64_t* act_out, float* logp_out, float* value_out) {
    ARG(c, "null"); JOIN(c); ARG(t >= 0 && t <= c->T, "t out of range");
    const StepSlice s = step_slice(c, -1);
    const bool have_rd = rew_prev != nullptr;
    if (rew_prev || done_prev) {
        ARG(rew_prev && done_prev && t >= 1, "rew_prev/done_prev come together and belong to step t-1");
        stage_rew_done(s, rew_prev, done_prev);
        if (c->gru_on) if (int r = done_to_gru(c, s)) return r;
    }
    InputSrc src{obs_ring(c), nullptr, (long long)t * s.n};
    const float* du;
    if (int r = upload_u(c, u, s.stream, 0, s.n, &du)) return r;
    c->prof.phase = 0;
    net_forward(c, src, s.n, {.recurrent = true, .heads = false});
    launch_step_heads(c, s, t, c->feat, du, seed, have_rd, ++c->roll_ticket);
    HIPC(hipGetLastError()); NETCHK(c);
    if (!wait_ticket(s.flag, c->roll_ticket, [&] { return hipStreamQuery(s.stream) != hipErrorNotReady; })) HIPC(hipStreamSynchronize(s.stream));
    unpack_step(s.h_pack, s.n, t == c->T, act_out, logp_out, value_out);
    return 0;
}

// ------------------------------------------------------------------------------------------ pipelined rollout (env groups)
// The reference's loop (agents/ppo.py:225-236) is strictly serial per step: obs -> H2D -> forward -> D2H act -> env.step.  An env's
// next frame depends only on its OWN action, so the E envs split into G contiguous groups whose chains
//     upload frames(t, g) -> forward + sample (t, g) -> actions on the host -> [env.step of group g on the host] -> upload frames(t+1, g)
// are independent: group g's upload (PCIe, ~37 us for 128 frames) and forward run on its stream while the host waits for / steps
// another group.  Per group (RolloutGroup, step_slice): its own stream, rows [e0, e0 + E/G) of the activation buffers, its slice of the
// pinned hand-off buffers, its own completion ticket.  Numbers are those of mi_rollout_step (same kernels, same Philox counters t*E + e).

// ---- rollout lanes (lanes.h): one registry per device, streams at the greatest priority the device offers.  The runtime keeps a pool of
// hardware queues per stream priority; the default stream, torch's streams and every context's own stream live in the normal pool, so
// the lanes are the only tenants of theirs and four of them sit on four queues even where the normal pool's four are all taken.
static LaneRegistry* const g_lanes = new LaneRegistry[MAX_LANE_DEVICES];      // (never destructed: a context may be destroyed during process exit)
static void* lane_make(int device, int, int* prio) {
    int dev0 = 0, least = 0, greatest = 0;
    hipStream_t s = nullptr;
    if (hipGetDevice(&dev0) != hipSuccess || hipSetDevice(device) != hipSuccess) return nullptr;
    const bool ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess &&
                    hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest) == hipSuccess &&
                    hipStreamGetPriority(s, prio) == hipSuccess;
    hipSetDevice(dev0);
    if (!ok && s) { hipStreamDestroy(s); s = nullptr; }
    return s;
}
static void lane_drop(void* s) { hipStreamDestroy((hipStream_t)s); }

int join_groups(mi_ctx* c) {
    for (int g = 0; g < c->n_groups; ++g) {
        RolloutGroup& G = c->grp[g];
        if (!G.stream) continue;
        if (G.worker) G.worker->drain();
        if (G.dirty) {
            HIPC(hipEventRecord(G.ev_join, G.stream));
            HIPC(hipStreamWaitEvent(c->main_stream, G.ev_join, 0));
            G.dirty = false;
        }
        G.forked = false;          // the next submit of this group orders itself behind the main stream again
    }
    c->groups_live = false;
    return 0;
}

// the device half of a group step, on the group's worker thread (tl_stream = the group's stream)
static int group_issue(mi_ctx* c, int g, const GroupJob& j) {
    const int E = c->E;
    const StepSlice s = step_slice(c, g);
    if (j.frames) {
        char* dst = obs_ring(c) + ((size_t)j.t * E + s.e0) * c->obs_bytes_per_env;
        // One upload at a time.  Uploads of several groups issued together share the PCIe link and all finish late and TOGETHER: the
        // groups' chains then stay in lock-step and every step pays the shared-link copy time (two stable regimes were measured at
        // E = 256, G = 4: 107 and 135-138 us per policy step).  Each upload reserves the link for bytes / rate from the moment the previous
        // reservation ends (a few us of spinning on the worker thread, only when groups bunch), which puts the chains out of step again.
        if (c->copy_rate_bytes_per_us > 0) {
            const int64_t gap = (int64_t)((double)j.bytes * 1000.0 / c->copy_rate_bytes_per_us);
            const auto clk = [] { return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
            int64_t slot = c->copy_slot_ns.load(), start;
            do { const int64_t now = clk(); start = now > slot ? now : slot; } while (!c->copy_slot_ns.compare_exchange_weak(slot, start + gap));
            while (clk() < start) __builtin_ia32_pause();
        }
        // page-locked, device-visible frames are PULLED by a kernel on the group's stream: a DMA copy in front of the first conv costs the
        // hand-over from the compute queue to the copy engine and back on top of the transfer (xfer.hip pull_i32_kernel)
        if (j.pull) launch_pull_bytes(j.frames, dst, j.bytes, s.stream);
        else HIPC(hipMemcpyAsync(dst, j.frames, j.bytes, hipMemcpyHostToDevice, s.stream));
    }
    if (j.have_rd && c->gru_on) if (int r = done_to_gru(c, s)) return r;      // (the hand-off rows were filled by the submitting thread)
    const float* du;
    if (int r = upload_u(c, j.u, s.stream, s.e0, s.n, &du)) return r;
    InputSrc src{obs_ring(c), nullptr, (long long)j.t * E + s.e0};
    net_forward(c, src, s.n, {.heads = false, .soff = s.e0});
    const float* hin = c->feat + (size_t)s.e0 * c->H;          // what the heads read: the embedder output, or h' of a GRU context
    if (c->gru_on) {
        // the GRU cell as ONE launch (gru_cell.hip gru_step_kernel): input state from hidden-ring slot t (mi_rec_begin's upload at t == 0, else
        // step t-1's output), masked by the group's done (mi_rec_begin's at t == 0, else the copy above); h' -> h_state rows, and slot t+1
        // unless this is the bootstrap step.  The heads read h' from h_state (the cell cannot overwrite feat, which its other workgroups read).
        const size_t H = c->H;
        float* slot = c->h_ring + ((size_t)j.t * E + s.e0) * H;
        launch_gru_step(c->feat + (size_t)s.e0 * H, slot, c->d_done + s.e0, c->gru_wih, c->gru_whh, c->gru_bih, c->gru_bhh, c->h_state + (size_t)s.e0 * H,
                        j.last ? nullptr : slot + (size_t)E * H, s.n, c->H, s.stream);
        hin = c->h_state + (size_t)s.e0 * H;
    }
    launch_step_heads(c, s, j.t, hin, du, j.seed, j.have_rd, j.ticket);
    HIPC(hipGetLastError());
    if (const char* lf = mi_launch_failed_take()) return fail(-4, lf);      // (this worker thread's launchers)
    return 0;
}
// what a group's worker (group_worker.h) runs per posted step, and the function its thread is started with
static int group_worker_run(mi_ctx* c, int g, const GroupJob& j, std::string* err) {
    const int rc = group_issue(c, g, j);
    if (rc) *err = g_err;
    return rc;
}
static void group_worker_main(mi_ctx* c, int g) {
    hipSetDevice(c->cfg.device);
    tl_stream = c->grp[g].stream;
    tl_ws_floats = c->gemm_ws_floats / mi_ctx::MAX_GROUPS; tl_ws = c->gemm_ws + (size_t)g * tl_ws_floats;     // concurrent groups: disjoint split-K slabs
    c->grp[g].worker->loop(c, g, group_worker_run);
}

int mi_rollout_groups(mi_ctx* c, int32_t n_groups) {
    ARG(c, "null"); ARG(n_groups >= 1 && n_groups <= mi_ctx::MAX_GROUPS, "1 .. 4 groups");
    ARG(c->E % n_groups == 0, "n_envs must be divisible by the number of groups");
    for (int g = 0; g < c->n_groups; ++g) ARG(!c->grp[g].busy, "a group step is still in flight: mi_rollout_wait it first");
    JOIN(c);
    void* lane[mi_ctx::MAX_GROUPS]; int prio[mi_ctx::MAX_GROUPS];
    const int have = [&] { int k = 0; while (k < mi_ctx::MAX_GROUPS && c->grp[k].stream) ++k; return k; }();
    if (n_groups > have && !g_lanes[c->cfg.device].borrow(c, n_groups, c->cfg.device, lane_make, lane, prio))
        return fail(-2, "no stream for an env group (hipStreamCreateWithPriority failed)");
    for (int g = 0; g < n_groups; ++g) {
        RolloutGroup& G = c->grp[g];
        if (G.stream) continue;
        DevPool::Group both(c->pool);
        HIPC(c->pool.event(&G.ev_fork, hipEventDisableTiming));
        HIPC(c->pool.event(&G.ev_join, hipEventDisableTiming));
        both.keep = true;
        G.stream = (hipStream_t)lane[g]; G.prio = prio[g];
        G.worker = new GroupWorker<GroupJob, mi_ctx>();
        G.worker->start(group_worker_main, c, g);
    }
    c->n_groups = n_groups;
    return 0;
}
// The groups' half of the context's teardown (ctx_release, in front of everything else it does): every worker stopped and deleted, then
// every group stream waited for.  The lanes themselves go back later, behind the main stream's wait and the profiler's harvest.
void rollout_groups_stop(mi_ctx* c) {
    for (RolloutGroup& G : c->grp)
        if (G.worker) { G.worker->stop(); delete G.worker; G.worker = nullptr; }
    for (RolloutGroup& G : c->grp) if (G.stream) hipStreamSynchronize(G.stream);
}
void rollout_lanes_return(mi_ctx* c) { g_lanes[c->cfg.device].give_back(c, lane_drop); }

int mi_rollout_lane_info(mi_ctx* c, int32_t* n, int32_t* prio, uint64_t* stream_id) {
    ARG(c && n && prio && stream_id, "null");
    *n = 0;
    for (int g = 0; g < c->n_groups && c->grp[g].stream; ++g) { prio[g] = c->grp[g].prio; stream_id[g] = (uint64_t)(uintptr_t)c->grp[g].stream; *n = g + 1; }
    return 0;
}

int mi_rollout_submit(mi_ctx* c, int32_t t, int32_t g, const void* frames, size_t bytes, const float* rew_prev, const float* done_prev,
                      uint64_t seed, const float* u) {
    ARG(c, "null"); ARG(t >= 0 && t <= c->T, "t out of range"); ARG(g >= 0 && g < c->n_groups, "group out of range");
    RolloutGroup& G = c->grp[g];
    ARG(G.stream, "call mi_rollout_groups first"); ARG(!G.busy, "this group's previous step has not been waited for");
    ARG(c->pending_n < 0, "a multirank minibatch is pending");
    const StepSlice s = step_slice(c, g);
    ARG(!frames || bytes == (size_t)s.n * c->obs_bytes_per_env, "frames byte count != (E / groups) * bytes_per_env");
    if (rew_prev || done_prev) ARG(rew_prev && done_prev && t >= 1, "rew_prev/done_prev come together and belong to step t-1");
    if (c->gru_on) {
        ARG(c->h_ring && (t > 0 || G.rec_ok), "recurrent rollout: call mi_rec_begin before the groups' first step (t == 0) of every rollout");
        if (t == 0) G.rec_ok = false;
    }
    G.worker->drain();
    if (!G.forked) {               // first step since the main stream last worked: parameters / packed banks must be in place
        fc_refresh(c);
        HIPC(hipEventRecord(G.ev_fork, c->main_stream));
        HIPC(hipStreamWaitEvent(G.stream, G.ev_fork, 0));
        G.forked = true;
    }
    c->groups_live = true; G.dirty = true;
    const bool have_rd = rew_prev != nullptr;
    if (have_rd) stage_rew_done(s, rew_prev, done_prev);
    const bool last = (t == c->T);
    bool pull = false;
    // Pull only what is latency-bound: measured per policy step, E = 64 in 2 groups (393 KB each) 73-76 us pulled vs 84-86 us copied,
    // E = 256 in 4 groups (786 KB each, four pulls competing) 121-135 vs 108-112 us -- shader reads of host memory move fewer bytes per
    // second than the copy engine, so above 512 KB the DMA's hand-over is the smaller price.
    if (frames && !c->no_pull && bytes <= (512u << 10) && (bytes & 15) == 0 && ((uintptr_t)frames & 15) == 0) {      // device-visible pinned memory? (asked once per buffer)
        auto it = c->pull_ok.find(frames);
        if (it == c->pull_ok.end()) {
            hipPointerAttribute_t at{};
            const bool ok = hipPointerGetAttributes(&at, frames) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer == frames;
            if (!ok) (void)hipGetLastError();
            if (c->pull_ok.size() > 64) c->pull_ok.clear();
            it = c->pull_ok.emplace(frames, ok).first;
        }
        pull = it->second;
    }
    G.worker->post(GroupJob{t, frames, bytes, pull, have_rd, last, u, seed, ++G.ticket});
    G.busy = true; G.last = last;
    return 0;
}

int mi_rollout_wait(mi_ctx* c, int32_t g, int64_t* act_out, float* logp_out, float* value_out) {
    ARG(c, "null"); ARG(g >= 0 && g < c->n_groups, "group out of range"); ARG(c->grp[g].busy, "nothing submitted for this group");
    RolloutGroup& G = c->grp[g];
    const StepSlice s = step_slice(c, g);
    const bool seen = wait_ticket(s.flag, G.ticket, [&] { return G.worker->idle() && hipStreamQuery(s.stream) != hipErrorNotReady; });   // issued, finished, no ticket
    G.worker->drain();
    G.busy = false;
    std::string why;
    if (const int rc = G.worker->take_error(&why)) return fail(rc, "group worker: " + why);
    if (!seen) HIPC(hipStreamSynchronize(s.stream));
    NETCHK(c);
    unpack_step(s.h_pack, s.n, G.last, act_out, logp_out, value_out);
    return 0;
}

// ------------------------------------------------------------------------------------------ staged entries
// What they share in front of their forward pass: the observations to the stage (bytes of them; want: what the entry takes), the caller's
// uniforms, if any, for the E rows -> where the network reads its input and the sampler its uniforms ...
static int stage_input(mi_ctx* c, const void* obs, size_t bytes, size_t want, const float* u, InputSrc* src, const float** du) {
    ARG(bytes == want, "obs byte count != E * bytes_per_env");
    void* stage = obs_stage(c);
    HIPC(hipMemcpyAsync(stage, obs, bytes, hipMemcpyHostToDevice, c->stream));
    if (int r = upload_u(c, u, c->stream, 0, c->E, du)) return r;
    *src = InputSrc{stage, nullptr, 0};
    return 0;
}
// ... and behind their launches: the staged act / logp / value (+ one more array) to the caller; mi_commit_staged may follow
static int hand_out_staged(mi_ctx* c, int64_t* act_out, float* logp_out, float* value_out, void* extra_out = nullptr, const void* d_extra = nullptr, size_t extra_bytes = 0) {
    if (int r = read_back_staged(c, c->s_act, c->s_logp, c->s_val, act_out, logp_out, value_out, extra_out, d_extra, extra_bytes)) return r;
    c->staged_valid = true;
    return 0;
}

int mi_predict_staged(mi_ctx* c, const void* obs, size_t bytes, uint64_t seed, uint64_t counter, const float* u,
                      int64_t* act_out, float* logp_out, float* value_out) {
    ARG(c && obs, "null"); JOIN(c);
    const int E = c->E;
    InputSrc src; const float* du;
    if (int r = stage_input(c, obs, bytes, (size_t)E * c->obs_bytes_per_env, u, &src, &du)) return r;
    net_forward(c, src, E, {.recurrent = true});
    launch_sample(c->hout, E, c->A, du, seed, counter, c->s_act, c->s_logp, c->s_val, c->stream, c->lse);
    HIPC(hipGetLastError()); NETCHK(c);
    return hand_out_staged(c, act_out, logp_out, value_out);
}

// IPL.predict(obs, greedy=True) (agents/IPL.py:82-94): mi_predict_staged with the first arg-max in place of the sampler
int mi_predict_greedy(mi_ctx* c, const void* obs, size_t bytes, int64_t* act_out, float* logp_out, float* value_out) {
    ARG(c && obs, "null"); JOIN(c);
    ARG(!c->gru_on, "mi_predict_greedy: a recurrent context (mi_set_gru) is not supported"); ARG(!c->lse, "mi_predict_greedy: value_from_logits is not supported");
    const int E = c->E;
    InputSrc src; const float* du;
    if (int r = stage_input(c, obs, bytes, (size_t)E * c->obs_bytes_per_env, nullptr, &src, &du)) return r;
    net_forward(c, src, E, {});
    launch_ipl_greedy(c->hout, E, c->A, c->s_act, c->s_logp, c->s_val, c->stream);
    HIPC(hipGetLastError()); NETCHK(c);
    return hand_out_staged(c, act_out, logp_out, value_out);
}

// PPO.predict_w_value_saliency (agents/ppo.py:83-94): predict + d value / d observation.  grad_out: IMPALA [E][64][64][3] (NHWC,
// wrt the k/255 float frames), MLP [E][obs_dim].  Runs the training-mode forward and the whole backward pass with dY = e_value on
// the E staged observations; the parameter gradients it produces on the way are discarded (the gradient buffer is zeroed again),
// so it must not be called between mi_minibatch and mi_optimizer_step of an accumulating update.
int mi_value_saliency(mi_ctx* c, const void* obs, size_t bytes, uint64_t seed, uint64_t counter, const float* u,
                      int64_t* act_out, float* logp_out, float* value_out, float* grad_out) {
    ARG(c && obs && grad_out, "null"); JOIN(c);
    ARG(c->pending_n < 0, "a multirank minibatch is pending");
    const int E = c->E;
    const bool impala = c->cfg.arch == MI_ARCH_IMPALA;
    InputSrc src; const float* du;
    if (int r = stage_input(c, obs, bytes, (size_t)E * c->obs_bytes_per_env, u, &src, &du)) return r;
    c->prof.phase = 0;
    const bool rec = c->gru_on;
    if (rec && !c->gru_x) { DevPool::Group both(c->pool); HIPC(c->pool.dev(&c->gru_x, (size_t)E * c->H)); HIPC(c->pool.dev(&c->gru_dg, (size_t)E * 3 * c->H)); both.keep = true; }
    net_forward(c, src, E, {.recurrent = rec, .train = true, .keep_gru_x = rec});          // recurrent: h' = GRU(embedder output, h (1 - done)) as a policy step does, heads on h'
    launch_sample(c->hout, E, c->A, du, seed, counter, c->s_act, c->s_logp, c->s_val, c->stream, c->lse);
    const float* g1;      // where the backward pass leaves the gradient of the first layer's output
    if (rec) {
        // value = w_v . h' + b_v: back through the GRU cell to its input x (common/model.py:219-225 under autograd, agents/ppo.py:88-89), then
        // through the embedder's final ReLU (IMPALA) -- d value / d x = dgates W_ih -- and on down the usual backward pass from dfeat
        // (value_from_logits: value = logsumexp(W_pi h' + b_pi), so the seed into the cell is per row, softmax(logits) W_pi; dfeat carries it)
        if (c->lse) {
            launch_lse_hidden_seed(c->hout, c->params + c->wh_off, c->dfeat, E, c->H, c->A, c->stream);
            launch_gru_value_bwd(c->gru_gi, c->gru_gh, c->h_masked, c->dfeat, c->gru_dg, E, c->H, c->stream, 1);
        } else
        launch_gru_value_bwd(c->gru_gi, c->gru_gh, c->h_masked, c->params + c->wh_off + (size_t)c->A * c->H, c->gru_dg, E, c->H, c->stream);
        linear_dgrad(c, c->gru_dg, c->gru_wih, impala ? c->gru_x : nullptr, c->dfeat, E, c->H, 3 * c->H);
        g1 = net_backward(c, src, E, {.from_dfeat = true});
    } else {
        if (c->lse) launch_lse_value_seed(c->hout, c->dY, E, c->A, c->stream);
        else launch_value_seed(c->dY, E, c->A, c->stream);
        g1 = net_backward(c, src, E, {});
    }
    ARG(g1, "backward did not reach the first layer");
    const size_t gfloats = impala ? (size_t)E * 64 * 64 * 3 : (size_t)E * c->cfg.obs_dim;
    if (!c->sal_dx) HIPC(c->pool.dev(&c->sal_dx, impala ? (size_t)c->NB * 64 * 64 * 3 : (size_t)c->NB * c->cfg.obs_dim));
    if (impala) {
        const void* dC = g1;
        if (c->bf) {                                       // the conv-output gradient is not materialised in bf16 mode: rebuild it from the pooled one
            if (!c->sal_dc) HIPC(c->pool.dev_raw(&c->sal_dc, (size_t)c->NB * 64 * 64 * 16 * 2 + 256));
            launch_maxpool_bwd_bf16(g1, c->blk[0].PI, c->sal_dc, E, 64, 16, c->stream);
            dC = c->sal_dc;
        }
        launch_conv1_input_grad(dC, c->bf, c->params + c->convs[0].w_off, c->sal_dx, E, c->stream);
    } else {
        linear_dgrad(c, g1, c->params + c->mlp[0].w_off, nullptr, c->sal_dx, E, c->mlp[0].in, c->mlp[0].out);
    }
    launch_fill(c->grads, c->n_params, 0.f, c->stream);    // discard the parameter gradients of this pass
    HIPC(hipGetLastError()); NETCHK(c);
    return hand_out_staged(c, act_out, logp_out, value_out, grad_out, c->sal_dx, gfloats * 4);
}

int mi_commit_staged(mi_ctx* c, int32_t t) {
    ARG(c, "null"); JOIN(c); ARG(t >= 0 && t <= c->T, "t out of range"); ARG(c->staged_valid, "nothing staged: call mi_predict_staged first");
    const size_t E = c->E, ob = E * c->obs_bytes_per_env;
    HIPC(hipMemcpyAsync(obs_ring(c) + (size_t)t * ob, obs_stage(c), ob, hipMemcpyDeviceToDevice, c->stream));
    if (t < c->T) {
        HIPC(hipMemcpyAsync(c->act + t * E, c->s_act, E * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPC(hipMemcpyAsync(c->logp + t * E, c->s_logp, E * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPC(hipMemcpyAsync(c->value + t * E, c->s_val, E * 4, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// log-probabilities of all actions, values and the embedder output (h' of a recurrent pass) of n observations; nothing stays staged
static int forward_common(mi_ctx* c, const void* obs, int32_t n, bool recurrent, float* logp_all, float* value, float* feat) {
    ARG(c && obs, "null"); JOIN(c); ARG(n >= 1 && n <= c->NB, "n must be in [1, max_batch]");
    c->staged_valid = false;
    InputSrc src; const float* du;
    const size_t bytes = (size_t)n * c->obs_bytes_per_env;
    if (int r = stage_input(c, obs, bytes, bytes, nullptr, &src, &du)) return r;
    net_forward(c, src, n, {.recurrent = recurrent});
    launch_logp_all(c->hout, n, c->A, c->d_lp, c->lse ? c->d_val : nullptr, c->stream, c->lse);
    HIPC(hipGetLastError()); NETCHK(c);
    if (logp_all) HIPC(hipMemcpyAsync(logp_all, c->d_lp, (size_t)n * c->A * 4, hipMemcpyDeviceToHost, c->stream));
    if (feat) HIPC(hipMemcpyAsync(feat, c->feat, (size_t)n * c->H * 4, hipMemcpyDeviceToHost, c->stream));
    std::vector<float> h;
    if (value && c->lse) HIPC(hipMemcpyAsync(value, c->d_val, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));      // (column A of hout is fc_value's output, not the value)
    else if (value) { h.resize((size_t)n * (c->A + 1)); HIPC(hipMemcpyAsync(h.data(), c->hout, h.size() * 4, hipMemcpyDeviceToHost, c->stream)); }
    HIPC(hipStreamSynchronize(c->stream));
    if (value && !c->lse) for (int k = 0; k < n; ++k) value[k] = h[(size_t)k * (c->A + 1) + c->A];
    return 0;
}
int mi_forward_rec(mi_ctx* c, const void* obs, float* logp_all, float* value, float* hidden_out) {
    ARG(c && obs, "null"); ARG(c->gru_on, "no GRU set");
    return forward_common(c, obs, c->E, true, logp_all, value, hidden_out);   // feat == h' after the GRU
}
int mi_forward(mi_ctx* c, const void* obs, int32_t n, float* logp_all, float* value, float* feat) {
    return forward_common(c, obs, n, false, logp_all, value, feat);
}

// ------------------------------------------------------------------------------------------ recurrent rollout: the GRU and its state
int mi_set_gru(mi_ctx* c, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh) {
    ARG(c && w_ih && w_hh && b_ih && b_hh, "null"); JOIN(c);
    const size_t H = c->H, E = c->E;
    if (!c->gru_wih) {
        DevPool& m = c->pool; DevPool::Group all(m);
        HIPC(m.dev(&c->gru_wih, 3 * H * H)); HIPC(m.dev(&c->gru_whh, 3 * H * H)); HIPC(m.dev(&c->gru_bih, 3 * H)); HIPC(m.dev(&c->gru_bhh, 3 * H));
        HIPC(m.dev(&c->h_state, E * H)); HIPC(m.dev(&c->h_masked, E * H)); HIPC(m.dev(&c->gru_gi, E * 3 * H)); HIPC(m.dev(&c->gru_gh, E * 3 * H));
        HIPC(m.dev(&c->d_done, E));
        all.keep = true;
    }
    const GruTensors g = gru_tensors(c);
    const float* src[4] = {w_ih, w_hh, b_ih, b_hh};
    for (int k = 0; k < 4; ++k) HIPC(hipMemcpy(g.t[k].p, src[k], g.t[k].len * 4, hipMemcpyHostToDevice));
    c->gru_on = true;
    return 0;
}
int mi_rec_state(mi_ctx* c, const float* hidden, const float* done) {
    ARG(c, "null"); JOIN(c); ARG(c->gru_on, "no GRU set: call mi_set_gru first");
    const size_t H = c->H, E = c->E;
    if (hidden) HIPC(hipMemcpyAsync(c->h_state, hidden, E * H * 4, hipMemcpyHostToDevice, c->stream));
    if (done) HIPC(hipMemcpyAsync(c->d_done, done, E * 4, hipMemcpyHostToDevice, c->stream));
    else HIPC(hipMemsetAsync(c->d_done, 0, E * 4, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_rec_begin(mi_ctx* c, const float* hidden, const float* done) {
    ARG(c, "null"); JOIN(c); ARG(c->gru_on, "no GRU set: call mi_set_gru first");
    const size_t H = c->H, E = c->E;
    if (!c->h_ring) {                                     // only contexts that run grouped recurrent rollouts pay for the ring (67 MB at T = E = H = 256)
        DevPool& m = c->pool; DevPool::Group all(m);
        HIPC(m.dev(&c->h_ring, (size_t)(c->T + 1) * E * H));
        HIPC(m.pinned(&c->h_rec_stage, (E * H + E) * 4, hipHostMallocDefault));
        HIPC(m.event(&c->ev_rec, hipEventDisableTiming));
        all.keep = true;
    } else
        HIPC(hipEventSynchronize(c->ev_rec));             // the previous call's upload has left the staging buffer (long since, normally)
    if (hidden) {
        memcpy(c->h_rec_stage, hidden, E * H * 4);
        HIPC(hipMemcpyAsync(c->h_ring, c->h_rec_stage, E * H * 4, hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemcpyAsync(c->h_state, c->h_ring, E * H * 4, hipMemcpyDeviceToDevice, c->stream));
    } else
        HIPC(hipMemcpyAsync(c->h_ring, c->h_state, E * H * 4, hipMemcpyDeviceToDevice, c->stream));
    if (done) {
        memcpy(c->h_rec_stage + E * H, done, E * 4);
        HIPC(hipMemcpyAsync(c->d_done, c->h_rec_stage + E * H, E * 4, hipMemcpyHostToDevice, c->stream));
    } else
        HIPC(hipMemsetAsync(c->d_done, 0, E * 4, c->stream));
    HIPC(hipEventRecord(c->ev_rec, c->stream));
    for (RolloutGroup& G : c->grp) G.rec_ok = true;
    return 0;
}
int mi_get_hidden_ring(mi_ctx* c, int32_t t0, int32_t t1, float* out) {
    ARG(c && out, "null"); JOIN(c); ARG(c->h_ring, "no hidden ring: mi_rec_begin has not run");
    ARG(t0 >= 0 && t0 < t1 && t1 <= c->T + 1, "need 0 <= t0 < t1 <= T + 1");
    const size_t slot = (size_t)c->E * c->H;
    HIPC(hipMemcpyAsync(out, c->h_ring + (size_t)t0 * slot, (size_t)(t1 - t0) * slot * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_get_hidden(mi_ctx* c, float* hidden) {
    ARG(c && hidden, "null"); JOIN(c); ARG(c->gru_on, "no GRU set");
    HIPC(hipMemcpyAsync(hidden, c->h_state, (size_t)c->E * c->H * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
