// The worker thread of one env group of the pipelined rollout and its one-slot mailbox: how the thread that calls mi_rollout_submit
// hands a step to the thread that issues the group's copies and launches, and how that thread's result comes back.
//
// This file is the hand-off only, plain C++ (the stand-alone host test runs it under the thread and address sanitizers with jobs that
// write into an array).  rollout.hip supplies the job type, the function the thread is started with (it sets the device and the
// thread-local stream / workspace overrides, then calls loop()) and the function that runs one job.  The protocol, one poster per worker:
//   post     job -> the slot, ++posted (seq_cst); only if the worker says it sleeps: lock-unlock its mutex, notify.  The poster has
//            drained the worker before, so the slot is free and rc / err are its to read.
//   loop     spin on posted for SPIN_BUDGET pauses (a rollout posts every ~30 us), then sleep on the condition variable until a post or
//            quit (the update phase: idle for tens of ms) -- SLEEP_MS bounds a sleep whatever happens; run the job; rc / err; done =
//            the post's number (release).
//   drain    spin until done == posted (acquire): everything posted has been issued, rc / err of the last job are visible.
//   stop     quit, lock-unlock, notify, join.  A job posted right before may or may not run.
// No allocation per post and no indirection but one function pointer: the loop runs 257 x G times per iteration inside the rollout's
// dependency chain.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>

template <typename Job, typename Ctx>
struct GroupWorker {
    typedef void (*MainFn)(Ctx* ctx, int id);                                        // the thread's function: what it needs set up, then loop()
    typedef int (*RunFn)(Ctx* ctx, int id, const Job& job, std::string* err);      // one job; non-zero: failed, *err says why
    static constexpr int SPIN_BUDGET = 40000, SLEEP_MS = 50;

    void start(MainFn main, Ctx* ctx, int id) { th = std::thread(main, ctx, id); }
    void post(const Job& j) {
        job = j;
        posted.fetch_add(1, std::memory_order_seq_cst);
        if (sleeping.load()) { { std::lock_guard<std::mutex> lk(mu); } cv.notify_one(); }
    }
    bool idle() const { return done.load() == posted.load(); }      // everything posted has been issued (a glance, no wait)
    void drain() const {
        while (done.load(std::memory_order_acquire) != posted.load(std::memory_order_acquire)) __builtin_ia32_pause();
    }
    // after drain(): the failure of the last job, handed out once (0: it went through)
    int take_error(std::string* why) {
        const int r = rc;
        if (r) { rc = 0; *why = err; }
        return r;
    }
    void stop() {
        if (!th.joinable()) return;
        quit.store(true); { std::lock_guard<std::mutex> lk(mu); } cv.notify_one();
        th.join();
    }
    ~GroupWorker() { stop(); }
    bool asleep() const { return sleeping.load(); }      // (what the host test looks at)
    // on the worker thread, until stop(): every posted job through run
    void loop(Ctx* ctx, int id, RunFn run) {
        unsigned seen = 0;
        for (;;) {
            int spins = 0;
            while (posted.load(std::memory_order_acquire) == seen && !quit.load()) {
                if (++spins < SPIN_BUDGET) __builtin_ia32_pause();
                else {                                   // idle for a few hundred us (update phase): sleep until the next post
                    std::unique_lock<std::mutex> lk(mu);
                    sleeping.store(true);
                    cv.wait_for(lk, std::chrono::milliseconds(SLEEP_MS), [&] { return posted.load() != seen || quit.load(); });
                    sleeping.store(false);
                    spins = 0;
                }
            }
            if (quit.load()) return;
            seen = posted.load(std::memory_order_acquire);
            rc = run(ctx, id, job, &err);
            done.store(seen, std::memory_order_release);
        }
    }

private:
    std::thread th; std::mutex mu; std::condition_variable cv;
    std::atomic<unsigned> posted{0}, done{0}; std::atomic<bool> sleeping{false}, quit{false};
    Job job{}; int rc = 0; std::string err;
};
