// Rollout lanes: the streams that serve the env groups of a pipelined rollout, shared by every context of the process on one device.
//
// Why they are not per context: the runtime hands hardware queues to streams out of one pool per stream priority, each pool as large
// as GPU_MAX_HW_QUEUES (default 4), and a queue shared by two group chains runs them strictly one after the other (DESIGN.md section
// 5, "Lanes").  Streams that every context created for itself -- on top of the default stream and the context's own -- outnumber the
// queues; four lanes per process, created at the greatest stream priority, have the high-priority pool to themselves.
//
// This file is the bookkeeping only, plain C++ over opaque handles (the stand-alone host test drives it with fake ones): which lanes
// exist, who holds which, which one a new group gets.  rollout.hip supplies the two callbacks that create and destroy a stream.
#pragma once
#include <mutex>
#include <utility>
#include <vector>

struct LaneRegistry {
    static constexpr int MAX_LANES = 4;
    typedef void* (*MakeFn)(int key, int lane, int* prio);      // a new stream for lane `lane` (null = failed) and its priority
    typedef void (*DropFn)(void* stream);

    // Owner `owner` wants `want` lanes in all (1 .. MAX_LANES; what it already holds stays where it is: a group never changes its
    // stream).  out[k] / prio[k], k < want: the stream and priority of the owner's k-th lane.  A new slot takes the lane with the fewest
    // holders among those the owner does not hold yet, the lowest index first: two owners of two lanes each get disjoint lanes, and
    // lanes are shared only when more groups are live than lanes exist.  Streams are created on first use.  Returns false when a
    // stream could not be created (the owner keeps the lanes it has got so far, until give_back).
    bool borrow(const void* owner, int want, int key, MakeFn make, void** out, int* prio) {
        std::lock_guard<std::mutex> lk(mu_);
        if (want < 1 || want > MAX_LANES) return false;
        Holder* h = find(owner);
        if (!h) { holders_.push_back(Holder{owner, {}}); h = &holders_.back(); }
        while ((int)h->lanes.size() < want) {
            int best = -1;
            for (int l = 0; l < MAX_LANES; ++l) {
                bool held = false;
                for (int x : h->lanes) held = held || x == l;
                if (!held && (best < 0 || lane_[l].users < lane_[best].users)) best = l;
            }
            Lane& L = lane_[best];
            if (!L.stream) {
                L.stream = make(key, best, &L.prio);
                if (!L.stream) { if (h->lanes.empty()) forget(owner); return false; }
            }
            ++L.users;
            h->lanes.push_back(best);
        }
        for (int k = 0; k < want; ++k) { out[k] = lane_[h->lanes[k]].stream; if (prio) prio[k] = lane_[h->lanes[k]].prio; }
        return true;
    }
    // The owner returns every lane it holds (its work on them has been waited for).  When nobody holds a lane any more the streams
    // are destroyed: the next first use starts from nothing, whatever earlier contexts created.
    void give_back(const void* owner, DropFn drop) {
        std::lock_guard<std::mutex> lk(mu_);
        Holder* h = find(owner);
        if (!h) return;
        for (int l : h->lanes) --lane_[l].users;
        forget(owner);
        if (!holders_.empty()) return;
        for (Lane& L : lane_) { if (L.stream) drop(L.stream); L = Lane{}; }
    }
    // ---- what the tests look at
    int users(int lane) { std::lock_guard<std::mutex> lk(mu_); return lane_[lane].users; }
    int live_streams() { std::lock_guard<std::mutex> lk(mu_); int n = 0; for (const Lane& L : lane_) n += L.stream != nullptr; return n; }
    int lane_of(const void* owner, int k) { std::lock_guard<std::mutex> lk(mu_); Holder* h = find(owner); return h && k < (int)h->lanes.size() ? h->lanes[k] : -1; }

private:
    struct Lane { void* stream = nullptr; int prio = 0; int users = 0; };
    struct Holder { const void* owner; std::vector<int> lanes; };
    Holder* find(const void* owner) { for (Holder& h : holders_) if (h.owner == owner) return &h; return nullptr; }
    void forget(const void* owner) { for (size_t i = 0; i < holders_.size(); ++i) if (holders_[i].owner == owner) { holders_.erase(holders_.begin() + i); return; } }
    std::mutex mu_;
    Lane lane_[MAX_LANES];
    std::vector<Holder> holders_;
};
