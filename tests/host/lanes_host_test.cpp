// Stand-alone host test of the rollout-lane bookkeeping (csrc/lanes.h) over fake stream handles: heap blocks, so that a sanitizer
// build reports a handle dropped twice, used after its drop, or never dropped.  Built and run by tests/test_lanes_host.py.
#include "../../train-procgen-pytorch_amd/csrc/lanes.h"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <thread>

static int g_made = 0, g_dropped = 0, g_fail_at = -1;
static void* make(int key, int lane, int* prio) {
    if (g_made == g_fail_at) return nullptr;
    int* h = new int[2]{key, lane};
    *prio = -1;
    ++g_made;
    return h;
}
static void drop(void* s) { delete[] (int*)s; ++g_dropped; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static std::set<void*> uniq(void** a, int n, void** b = nullptr, int m = 0) {
    std::set<void*> s(a, a + n);
    if (b) s.insert(b, b + m);
    return s;
}

int main() {
    int A, B, C;          // owners: any distinct addresses
    void *a[4], *b[4], *c[4];
    int pr[4];
    {   // borrow 4, return: created on first use, destroyed when the last holder goes
        LaneRegistry R;
        CHECK(R.live_streams() == 0);
        CHECK(R.borrow(&A, 4, 7, make, a, pr) && uniq(a, 4).size() == 4 && g_made == 4 && pr[3] == -1);
        for (int k = 0; k < 4; ++k) { CHECK(((int*)a[k])[0] == 7 && ((int*)a[k])[1] == k && R.users(k) == 1 && R.lane_of(&A, k) == k); }
        void* again[4];
        CHECK(R.borrow(&A, 4, 7, make, again, pr) && g_made == 4);          // asking again changes nothing
        for (int k = 0; k < 4; ++k) CHECK(again[k] == a[k]);
        CHECK(R.borrow(&A, 2, 7, make, again, pr) && again[0] == a[0] && again[1] == a[1] && R.users(3) == 1);      // fewer groups: the lanes stay held
        R.give_back(&A, drop);
        CHECK(g_dropped == 4 && R.live_streams() == 0);
        R.give_back(&A, drop);                                               // a second return is a no-op
        CHECK(g_dropped == 4);
    }
    {   // 2 + 2 from two owners: disjoint; one returns, a third owner with 4 gets four different lanes, two of them shared
        LaneRegistry R;
        g_made = g_dropped = 0;
        CHECK(R.borrow(&A, 2, 0, make, a, pr) && R.borrow(&B, 2, 0, make, b, pr));
        CHECK(uniq(a, 2, b, 2).size() == 4 && g_made == 4);
        R.give_back(&A, drop);
        CHECK(g_dropped == 0 && R.live_streams() == 4);                      // B still holds lanes: nothing is destroyed
        CHECK(R.users(0) == 0 && R.users(1) == 0 && R.users(2) == 1 && R.users(3) == 1);
        CHECK(R.borrow(&C, 4, 0, make, c, pr) && uniq(c, 4).size() == 4 && g_made == 4);
        CHECK(c[0] == a[0] && c[1] == a[1]);                                 // the free lanes first
        CHECK(R.users(0) == 1 && R.users(1) == 1 && R.users(2) == 2 && R.users(3) == 2);
        // grow: an owner of 2 asks for 4 and keeps its first two
        void* b4[4];
        CHECK(R.borrow(&B, 4, 0, make, b4, pr) && b4[0] == b[0] && b4[1] == b[1] && uniq(b4, 4).size() == 4);
        for (int k = 0; k < 4; ++k) CHECK(R.users(k) == 2);                   // over-subscribed 4 + 4: every lane shared by two
        R.give_back(&C, drop); R.give_back(&B, drop);
        CHECK(g_dropped == 4 && R.live_streams() == 0);
        // history: what comes after starts from nothing
        CHECK(R.borrow(&A, 1, 0, make, a, pr) && g_made == 5 && R.lane_of(&A, 0) == 0 && R.live_streams() == 1);
        R.give_back(&A, drop);
        CHECK(g_dropped == 5);
    }
    {   // a stream that cannot be created: reported, nothing leaks, the registry stays usable
        LaneRegistry R;
        g_made = g_dropped = 0; g_fail_at = 2;
        CHECK(!R.borrow(&A, 4, 0, make, a, pr) && g_made == 2);
        CHECK(!R.borrow(&B, 0, 0, make, b, pr) && !R.borrow(&B, 5, 0, make, b, pr));
        g_fail_at = -1;
        CHECK(R.borrow(&A, 4, 0, make, a, pr) && g_made == 4 && uniq(a, 4).size() == 4);
        R.give_back(&A, drop);
        CHECK(g_dropped == 4);
    }
    {   // owners on four threads (the engine's entry points may be called from several)
        LaneRegistry R;
        g_made = g_dropped = 0;
        int own[4];
        std::thread th[4];
        for (int i = 0; i < 4; ++i)
            th[i] = std::thread([&R, &own, i] {
                for (int rep = 0; rep < 200; ++rep) {
                    void* s[4]; int p[4];
                    if (!R.borrow(&own[i], 1 + (i + rep) % 4, 0, make, s, p)) abort();
                    R.give_back(&own[i], drop);
                }
            });
        for (auto& t : th) t.join();
        CHECK(R.live_streams() == 0 && g_made == g_dropped);
    }
    printf("lanes host test OK\n");
    return 0;
}
