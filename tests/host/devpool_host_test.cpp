// Stand-alone host test of the owning resource pool (csrc/devpool.h) over a fake backend: handles are heap blocks, so that a sanitizer
// build reports one that is destroyed twice, used after its release, or never released.  The backend can be told to fail at its k-th
// acquiring call; the same sequence runs for every k.  Built and run by tests/test_devpool_host.py.
#include "../../train-procgen-pytorch_amd/csrc/devpool.h"
#include <cstdio>
#include <cstdlib>
#include <set>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d (fail_at %d): %s\n", __LINE__, g_fail_at, #x); exit(1); } } while (0)

enum { DEV = 0, PINNED = 1, EVENT = 2 };
struct Handle { int kind, seq; size_t bytes; unsigned flags; bool zero; };
static int g_fail_at = -1, g_calls = 0, g_made = 0, g_destroyed = 0;
static std::set<Handle*> g_live;
static int live(int kind) { int n = 0; for (Handle* h : g_live) n += h->kind == kind; return n; }

static int make(int kind, void** p, size_t bytes, unsigned flags, bool zero) {
    const int call = g_calls++;
    if (call == g_fail_at) { *p = (void*)0x1; return 1000 + call; }      // (a failing call may scribble on the pointer; the pool must null it)
    Handle* h = new Handle{kind, g_made++, bytes, flags, zero};
    g_live.insert(h);
    *p = h;
    return 0;
}
static void unmake(int kind, void* p) {
    Handle* h = (Handle*)p;
    CHECK(g_live.count(h) == 1);                                         // created, and not destroyed before
    CHECK(h->kind == kind);                                              // through the free function of its own kind
    for (Handle* o : g_live) CHECK(o->seq <= h->seq);                    // the newest one still held: reverse order of creation
    g_live.erase(h);
    ++g_destroyed;
    delete h;
}
static int dev_alloc(void** p, size_t bytes, bool zero) { return make(DEV, p, bytes, 0, zero); }
static void dev_free(void* p) { unmake(DEV, p); }
static int pinned_alloc(void** p, size_t bytes, unsigned flags) { return make(PINNED, p, bytes, flags, false); }
static void pinned_free(void* p) { unmake(PINNED, p); }
static int event_create(void** e, unsigned flags) { return make(EVENT, e, 0, flags, false); }
static void event_destroy(void* e) { unmake(EVENT, e); }
static const DevPool::Backend kFake = {dev_alloc, dev_free, pinned_alloc, pinned_free, event_create, event_destroy};

// what an owner looks like: pointers of several types, filled in a fixed order
static constexpr int N = 36;
struct Owner { void* slot[N] = {}; };
static int acquire(DevPool& m, Owner& o, int i) {
    switch (i % 6) {
        case 0: return m.dev((float**)&o.slot[i], 10 + i);
        case 1: return m.pinned((int**)&o.slot[i], 64 + i, 0x40000002u + i);
        case 2: return m.event((Handle**)&o.slot[i], 2u);
        case 3: return m.dev((double**)&o.slot[i], 3);
        case 4: return m.dev_raw(&o.slot[i], 100 + i);
        default: return m.dev((unsigned char**)&o.slot[i], 0);
    }
}
static void check_handle(const Owner& o, int i) {
    const Handle* h = (const Handle*)o.slot[i];
    CHECK(h && g_live.count((Handle*)h) == 1);
    switch (i % 6) {
        case 0: CHECK(h->kind == DEV && h->bytes == (10 + i) * sizeof(float) + 256 && h->zero); break;
        case 1: CHECK(h->kind == PINNED && h->bytes == (size_t)64 + i && h->flags == 0x40000002u + i); break;
        case 2: CHECK(h->kind == EVENT && h->flags == 2u); break;
        case 3: CHECK(h->kind == DEV && h->bytes == 3 * sizeof(double) + 256 && h->zero); break;
        case 4: CHECK(h->kind == DEV && h->bytes == (size_t)100 + i && !h->zero); break;
        default: CHECK(h->kind == DEV && h->bytes == 256 && h->zero); break;
    }
}
// slots [i, end) in order; stops at the first failure
static int take(DevPool& m, Owner& o, int& i, int end) {
    for (; i < end; ++i)
        if (int e = acquire(m, o, i)) return e;
    return 0;
}
// A lazily allocated group, slots [first, end): transactional.  A failure inside leaves the owner as it was before the call and the
// second call gets it all.
static void lazy_group(DevPool& m, Owner& o, int first, int end) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int made0 = g_made, destroyed0 = g_destroyed, calls0 = g_calls;
        const size_t live0 = g_live.size();
        int i = first, e;
        {
            DevPool::Group g(m);
            e = take(m, o, i, end);
            g.keep = e == 0;
        }
        if (!e) { CHECK(g_made - made0 == end - first && g_destroyed == destroyed0); return; }
        CHECK(attempt == 0);                                             // (the backend fails once per run)
        CHECK(e == 1000 + g_fail_at && g_fail_at == calls0 + (i - first));  // the backend's own error, from the call that failed
        CHECK(g_destroyed - destroyed0 == g_made - made0 && g_live.size() == live0);      // exactly what the group had got so far
        for (int k = first; k < end; ++k) CHECK(o.slot[k] == nullptr);   // the group's pointers are null again
        for (int k = 0; k < first; ++k) check_handle(o, k);              // everything earlier is still held
    }
}

// create (12) + lazy group A (7) + 5 more + lazy group B (8) + 4 more = N acquisitions; fail_at == N: nothing fails
static void run(int fail_at) {
    g_fail_at = fail_at; g_calls = g_made = g_destroyed = 0;
    Owner o;
    {
        DevPool m(&kFake);
        CHECK(m.mark() == 0);
        int i = 0;
        int e = take(m, o, i, 12);
        if (e) {                                                          // a create that fails: the caller releases everything
            CHECK(e == 1000 + fail_at && i == fail_at && o.slot[i] == nullptr && (int)m.mark() == i);
        } else {
            lazy_group(m, o, 12, 19);
            i = 19; e = take(m, o, i, 24);
            if (e) { CHECK(e == 1000 + fail_at && o.slot[i] == nullptr); ++i; CHECK(take(m, o, i, 24) == 0); }      // a single buffer: simply absent
            lazy_group(m, o, 24, 32);
            i = 32; e = take(m, o, i, N);
            if (e) CHECK(e == 1000 + fail_at && o.slot[i] == nullptr);
            for (int k = 0; k < i; ++k) if (o.slot[k]) check_handle(o, k);
            if (fail_at >= N) { CHECK(g_made == N && (int)m.mark() == N && live(DEV) == 24 && live(PINNED) == 6 && live(EVENT) == 6); }
        }
        CHECK(g_live.size() == m.mark());
        m.release_all();
        CHECK(g_live.empty() && live(DEV) + live(PINNED) + live(EVENT) == 0 && g_destroyed == g_made && m.mark() == 0);
        for (int k = 0; k < N; ++k) CHECK(o.slot[k] == nullptr);
        m.release_all();                                                  // a second release does nothing more
        CHECK(g_destroyed == g_made);
    }
    CHECK(g_destroyed == g_made && g_live.empty());                       // nor does the destructor
}

int main() {
    for (int k = 0; k <= N; ++k) run(k);
    {   // the destructor alone releases, and a rollback to a mark keeps what is older
        g_fail_at = -1; g_calls = g_made = g_destroyed = 0;
        Owner o;
        {
            DevPool m(&kFake);
            int i = 0;
            CHECK(take(m, o, i, 5) == 0);
            const size_t mk = m.mark();
            CHECK(take(m, o, i, 9) == 0 && g_live.size() == 9);
            m.rollback(mk);
            CHECK(g_live.size() == 5 && g_destroyed == 4 && o.slot[4] && !o.slot[5] && !o.slot[8]);
        }
        CHECK(g_live.empty() && g_destroyed == 9 && !o.slot[0]);
    }
    printf("devpool host test OK\n");
    return 0;
}
