// Owning pool of an engine context's device resources: device buffers, pinned host buffers and events.  Whoever acquires through a
// pool never frees by hand: release_all() (and the destructor) gives everything back in reverse order of acquisition, exactly once,
// however far the owner's construction got.  Streams are not pooled: each of the context's three has a rule of its own.
//
// A lazily allocated group of buffers is acquired inside a Group scope: unless the scope is kept, everything acquired since it opened
// is released again and the caller's pointers are null again, so a failed first call leaves the owner as if it had never been made
// and the next call retries.
//
// This file is the bookkeeping only, plain C++ over opaque handles (the stand-alone host test drives it with a fake backend).
// engine.hip supplies the HIP backend.  A pool is used by one thread at a time, like the context that owns it.
#pragma once
#include <stddef.h>
#include <vector>

struct DevPool {
    // Every function returns 0 or the backend's own error code, which the pool's calls pass on unchanged.
    struct Backend {
        int (*dev_alloc)(void** p, size_t bytes, bool zero);      // zero: zero-filled, the fill complete before the call returns
        void (*dev_free)(void* p);
        int (*pinned_alloc)(void** p, size_t bytes, unsigned flags);
        void (*pinned_free)(void* p);
        int (*event_create)(void** e, unsigned flags);
        void (*event_destroy)(void* e);
    };
    static constexpr size_t PAD = 256;      // behind every typed device buffer: covers the kernels' vector over-reads

    explicit DevPool(const Backend* be) : be_(be) {}
    ~DevPool() { release_all(); }
    DevPool(const DevPool&) = delete;
    DevPool& operator=(const DevPool&) = delete;

    // `count` elements + PAD bytes of device memory, zero-filled; the fill is complete, so the caller may launch on it at once
    template <typename T> int dev(T** p, size_t count) { return took(DEV, (void**)p, be_->dev_alloc((void**)p, count * sizeof(T) + PAD, true)); }
    // `bytes` of device memory as the allocator hands them out (no padding, no fill)
    template <typename T> int dev_raw(T** p, size_t bytes) { return took(DEV, (void**)p, be_->dev_alloc((void**)p, bytes, false)); }
    template <typename T> int pinned(T** p, size_t bytes, unsigned flags) { return took(PINNED, (void**)p, be_->pinned_alloc((void**)p, bytes, flags)); }
    template <typename E> int event(E* e, unsigned flags) { return took(EVENT, (void**)e, be_->event_create((void**)e, flags)); }      // E: a pointer-sized handle

    void release_all() { rollback(0); }
    size_t mark() const { return held_.size(); }
    // release what was acquired since mark() returned `m`, newest first, and null the pointers it was handed out through
    void rollback(size_t m) {
        while (held_.size() > m) {
            const Held h = held_.back();
            held_.pop_back();
            (h.kind == DEV ? be_->dev_free : h.kind == PINNED ? be_->pinned_free : be_->event_destroy)(h.handle);
            *h.slot = nullptr;
        }
    }
    struct Group {
        DevPool& pool; size_t m; bool keep = false;
        explicit Group(DevPool& p) : pool(p), m(p.mark()) {}
        ~Group() { if (!keep) pool.rollback(m); }
    };

private:
    enum Kind { DEV, PINNED, EVENT };
    struct Held { Kind kind; void* handle; void** slot; };      // slot: the owner's pointer (it outlives the pool's hold on the handle)
    int took(Kind k, void** slot, int err) {
        if (err) *slot = nullptr; else held_.push_back(Held{k, *slot, slot});
        return err;
    }
    const Backend* be_;
    std::vector<Held> held_;
};
