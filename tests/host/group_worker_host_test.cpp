// Stand-alone host test of the env-group worker's hand-off (csrc/group_worker.h) without a GPU: posting threads hand jobs that write
// into disjoint rows of a shared array to up to four workers.  Built with the thread sanitizer and with the address + undefined-
// behaviour sanitizers and run once each by tests/test_group_worker_host.py.
#include "../../train-procgen-pytorch_amd/csrc/group_worker.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

struct Job { int k; bool fail; long long payload[4]; };
static Job make_job(int k) { return Job{k, k % 7 == 3 || k % 50 == 49, {k, 3LL * k + 1, ~(long long)k, 1LL << (k % 60)}}; }
static bool same(const Job& a, const Job& b) {
    return a.k == b.k && a.fail == b.fail && a.payload[0] == b.payload[0] && a.payload[1] == b.payload[1] && a.payload[2] == b.payload[2] && a.payload[3] == b.payload[3];
}
static int rc_of(int id, int k) { return make_job(k).fail ? -(1 + (k + id) % 5) : 0; }
static std::string err_of(int id, int k) { return "job " + std::to_string(k) + " of worker " + std::to_string(id); }

struct Shared;
typedef GroupWorker<Job, Shared> Worker;
static constexpr int W_MAX = 4;
struct Shared {
    Worker* w[W_MAX] = {};                  // worker id, as its thread's function finds it
    int n_jobs = 0;
    std::vector<int> cell[W_MAX];          // cell[id][k]: how often job k of worker id ran (plain ints: only worker id writes row id)
    int next[W_MAX] = {};                   // the job worker id expects next
    int inits[W_MAX] = {};
    std::thread::id tid[W_MAX];
    std::atomic<int> bad{0};
};
static int run(Shared* s, int id, const Job& j, std::string* err);
static void thread_main(Shared* s, int id) { ++s->inits[id]; s->tid[id] = std::this_thread::get_id(); s->w[id]->loop(s, id, run); }
static void start(Shared* s, Worker* w, int id) { s->w[id] = w; w->start(thread_main, s, id); }
static int run(Shared* s, int id, const Job& j, std::string* err) {
    if (!same(j, make_job(j.k)) || j.k != s->next[id] || s->tid[id] != std::this_thread::get_id() || s->inits[id] != 1) s->bad.fetch_add(1);
    if (j.k >= 0 && j.k < s->n_jobs) ++s->cell[id][j.k];
    ++s->next[id];
    if (j.fail) *err = err_of(id, j.k);
    return rc_of(id, j.k);
}

static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
static void wait_asleep(const Worker& w) {          // idle longer than the spin budget: the worker says it sleeps
    const auto t0 = std::chrono::steady_clock::now();
    while (!w.asleep()) { CHECK(ms_since(t0) < 20000.0); std::this_thread::sleep_for(std::chrono::microseconds(200)); }
}
static void expect_error(Worker& w, int id, int k) {          // after drain: job k's result, handed out once
    std::string why = "untouched";
    const int rc = w.take_error(&why);
    CHECK(rc == rc_of(id, k));
    CHECK(rc ? why == err_of(id, k) : why == "untouched");
    CHECK(w.take_error(&why) == 0);
}

// one posting thread serves workers first, first + stride, ...: job k goes to each of them before job k + 1 does
static void poster(Shared* s, Worker* w, int first, int stride, int n_workers, std::vector<double>* wake_ms) {
    std::vector<bool> checked(W_MAX, true);          // job k - 1's result has been looked at
    for (int k = 0; k < s->n_jobs; ++k)
        for (int id = first; id < n_workers; id += stride) {
            w[id].drain();
            CHECK(w[id].idle());
            if (!checked[id]) expect_error(w[id], id, k - 1);
            const bool nap = k > 0 && k % (s->n_jobs / 20) == 0;
            if (nap) wait_asleep(w[id]);
            const auto t0 = std::chrono::steady_clock::now();
            w[id].post(make_job(k));
            checked[id] = false;
            if (nap || k % 3 == 0) {          // the result right away
                w[id].drain();
                if (nap) wake_ms->push_back(ms_since(t0));
                expect_error(w[id], id, k);
                checked[id] = true;
            }
        }
    for (int id = first; id < n_workers; id += stride) {
        w[id].drain();
        if (!checked[id]) expect_error(w[id], id, s->n_jobs - 1);
    }
}

static void hand_off(int n_posters, int n_workers, int n_jobs) {
    Shared s;
    s.n_jobs = n_jobs;
    for (int id = 0; id < n_workers; ++id) s.cell[id].assign(n_jobs, 0);
    std::vector<double> wake[2];
    {
        Worker w[W_MAX];
        for (int id = 0; id < n_workers; ++id) start(&s, &w[id], id);
        std::thread second;
        if (n_posters == 2) second = std::thread(poster, &s, w, 1, 2, n_workers, &wake[1]);
        poster(&s, w, 0, n_posters, n_workers, &wake[0]);
        if (second.joinable()) second.join();
        for (int id = 0; id < n_workers; ++id) w[id].stop();
        for (int id = 0; id < n_workers; ++id) w[id].stop();          // (again: nothing left to do)
    }
    CHECK(s.bad.load() == 0);
    for (int id = 0; id < n_workers; ++id) {
        CHECK(s.next[id] == n_jobs && s.inits[id] == 1);
        for (int k = 0; k < n_jobs; ++k) CHECK(s.cell[id][k] == 1);
    }
    // A sleeping worker wakes on the post, not on the end of its SLEEP_MS: a worker that only its timeout woke would need half of it on
    // average.  The median over the naps of a posting thread keeps a descheduled thread or a slow sanitizer run from deciding it.
    for (int p = 0; p < n_posters; ++p) {
        std::vector<double>& v = wake[p];
        CHECK(v.size() >= 19);
        std::sort(v.begin(), v.end());
        printf("posters %d workers %d: post -> done of a sleeping worker, median %.3f ms, worst %.3f ms over %zu naps\n", n_posters, n_workers, v[v.size() / 2], v.back(), v.size());
        CHECK(v[v.size() / 2] < 0.4 * Worker::SLEEP_MS);
    }
}

static void stops() {
    Shared s;
    s.n_jobs = 1;
    { Worker never_started; }
    for (int id = 0; id < W_MAX; ++id) s.cell[id].assign(1, 0);
    { Worker w; start(&s, &w, 0); w.stop(); CHECK(s.next[0] == 0); }                       // nothing ever posted
    { Worker w; start(&s, &w, 1); }                                                        // ... and left to the destructor
    { Worker w; start(&s, &w, 2); wait_asleep(w); w.stop(); CHECK(s.next[2] == 0); }       // a sleeping worker
    CHECK(s.inits[0] == 1 && s.inits[1] == 1 && s.inits[2] == 1);
    int ran = 0;
    for (int k = 0; k < 300; ++k) {          // right after a post: the job runs or it does not, and stop() returns
        Shared t;
        t.n_jobs = 1; t.cell[3].assign(1, 0);
        Worker w;
        start(&t, &w, 3);
        if (k % 3 == 1) wait_asleep(w);
        if (k % 3 == 2) std::this_thread::sleep_for(std::chrono::microseconds(50));
        w.post(make_job(0));
        w.stop();
        CHECK(t.bad.load() == 0 && (t.next[3] == 0 || t.next[3] == 1) && t.cell[3][0] == t.next[3]);
        ran += t.next[3];
    }
    printf("stop right after a post: the job ran in %d of 300\n", ran);
}

int main() {
    hand_off(1, 1, 3000);
    hand_off(1, 3, 2000);
    hand_off(2, 4, 3000);
    stops();
    printf("group worker host test OK\n");
    return 0;
}
