// Stand-alone test of fedtree_amd/csrc/group_commit.hpp: the group-commit queue of the fthe_*_shared calls with a
// fake runner, no GPU and no libfthe.  Build and sanitizer command lines: tools/README.md;
// tests/test_group_commit.py builds and runs it plain.  Prints "group commit OK" and exits 0, or says what failed.
#include "../fedtree_amd/csrc/group_commit.hpp"

#include <atomic>
#include <cstdio>
#include <new>
#include <thread>
#include <sys/wait.h>
#include <unistd.h>

#if defined(__SANITIZE_THREAD__)
// Thread-sanitizer builds only.  libstdc++'s wait_for on the steady clock calls pthread_cond_clockwait, which g++ 11's
// sanitizer runtime does not intercept: it then misses the wait's unlock and relock of the mutex and reports double
// locks and races on everything that mutex guards.  Route the call to pthread_cond_timedwait, which it does intercept.
#include <pthread.h>
#include <time.h>
extern "C" int pthread_cond_clockwait(pthread_cond_t *cond, pthread_mutex_t *mutex, clockid_t clock,
                                      const struct timespec *abstime) {
    struct timespec now, real;
    clock_gettime(clock, &now);
    clock_gettime(CLOCK_REALTIME, &real);
    int64_t ns = (int64_t)(abstime->tv_sec - now.tv_sec) * 1000000000 + (abstime->tv_nsec - now.tv_nsec);
    ns = std::max<int64_t>(ns, 0) + real.tv_nsec;
    real.tv_sec += ns / 1000000000; real.tv_nsec = ns % 1000000000;
    return pthread_cond_timedwait(cond, mutex, &real);
}
#endif

namespace {

int failures = 0;
std::mutex fail_mu;
#define CHECK(cond, ...)                                                 \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::lock_guard<std::mutex> g_(fail_mu);                     \
            if (failures++ < 20) {                                       \
                std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);                       \
                std::fprintf(stderr, "\n");                              \
            }                                                            \
        }                                                                \
    } while (0)

struct Req {
    uint64_t in; int key; bool poison;
    uint64_t out = 0;
    int seen = 0;                // times a runner saw this request
    bool thrown = false;         // it was part of the batch that threw
    int rc = FTHE_OK; bool done = false;
};

uint64_t result_of(uint64_t in, int key) { return in * 0x9E3779B97F4A7C15ull + (uint64_t)key; }

// One queue and its fake runner: every request's result from its input, group by group.
struct Queue {
    GroupCommit<Req> gc;
    std::atomic<int> in_flight{0}, max_in_flight{0};
    std::atomic<size_t> batches{0}, batched{0}, thrown_batches{0}, largest{0};
    // the last check of main(): a runner stays in flight until the other queue's runner has entered too, so the one
    // that enters second finds the first still running
    std::atomic<bool> entered{false}, met{false};
    std::atomic<bool> *other_entered = nullptr;

    void run(const std::vector<Req *> &batch) {
        const int now = ++in_flight;
        int mx = max_in_flight.load();
        while (now > mx && !max_in_flight.compare_exchange_weak(mx, now)) {}
        struct Leave { std::atomic<int> &n; ~Leave() { --n; } } leave{in_flight};
        batches++; batched += batch.size();
        size_t lg = largest.load();
        while (batch.size() > lg && !largest.compare_exchange_weak(lg, batch.size())) {}
        if (other_entered) {
            entered = true;
            const auto t0 = std::chrono::steady_clock::now();
            while (!other_entered->load() && us_since(t0) < 10 * 1000000) std::this_thread::yield();
            met = other_entered->load();
        }
        bool poison = false;
        for (Req *r : batch) { r->seen++; poison |= r->poison; }
        if (poison) {
            for (Req *r : batch) r->thrown = true;
            thrown_batches++;
            throw std::bad_alloc();
        }
        size_t members = 0;
        for (const auto &grp : group_by_key(batch, [](const Req &r) { return r.key; }))
            for (Req *r : grp.second) {
                CHECK(r->key == grp.first, "request of key %d in group %d", r->key, grp.first);
                r->out = result_of(r->in, r->key); r->rc = FTHE_OK; members++;
            }
        CHECK(members == batch.size(), "%zu of %zu requests grouped", members, batch.size());
    }
    int call(Req &r) {
        return gc.submit(r, [this](const std::vector<Req *> &batch) { run(batch); });
    }
};

void check_grouping() {
    Req rs[6] = {{0, 2, false}, {1, 1, false}, {2, 2, false}, {3, 3, false}, {4, 1, false}, {5, 2, false}};
    std::vector<Req *> batch;
    for (Req &r : rs) batch.push_back(&r);
    const auto groups = group_by_key(batch, [](const Req &r) { return r.key; });
    const int keys[3] = {2, 1, 3};
    const std::vector<uint64_t> members[3] = {{0, 2, 5}, {1, 4}, {3}};
    CHECK(groups.size() == 3, "%zu groups", groups.size());
    for (size_t g = 0; g < groups.size() && g < 3; g++) {
        CHECK(groups[g].first == keys[g], "group %zu has key %d", g, groups[g].first);
        std::vector<uint64_t> got;
        for (const Req *r : groups[g].second) got.push_back(r->in);
        CHECK(got == members[g], "group %zu: members out of batch order", g);
    }
}

// kThreads threads make kCalls calls each on q with mixed keys; call (poison_thread, poison_call)'s batch throws.
constexpr int kThreads = 24, kCalls = 200;
void drive(Queue &q, std::vector<std::thread> &ths, int poison_thread, int poison_call, std::atomic<int> &nomem) {
    for (int t = 0; t < kThreads; t++)
        ths.emplace_back([&q, &nomem, t, poison_thread, poison_call] {
            for (int j = 0; j < kCalls; j++) {
                Req r{(uint64_t)t * kCalls + j, (t + j) % 3, t == poison_thread && j == poison_call};
                const int rc = q.call(r);
                CHECK(r.done && rc == r.rc, "thread %d call %d: rc %d, request says %d", t, j, rc, r.rc);
                CHECK(r.seen == 1, "thread %d call %d seen by %d runners", t, j, r.seen);
                if (r.thrown) {
                    CHECK(rc == FTHE_ERR_NOMEM, "thread %d call %d in the throwing batch: rc %d", t, j, rc);
                    nomem++;
                } else {
                    CHECK(rc == FTHE_OK, "thread %d call %d: rc %d", t, j, rc);
                    CHECK(r.out == result_of(r.in, r.key), "thread %d call %d got another caller's result", t, j);
                }
            }
        });
}

void check_queue(const char *name, Queue &q, size_t calls, size_t thrown, int nomem) {
    CHECK(q.batched == calls, "%s: batches sum to %zu of %zu calls", name, q.batched.load(), calls);
    CHECK(q.max_in_flight == 1, "%s: %d leaders at once", name, q.max_in_flight.load());
    CHECK(q.thrown_batches == thrown, "%s: %zu batches threw", name, q.thrown_batches.load());
    CHECK((thrown == 0) == (nomem == 0), "%s: %d calls returned FTHE_ERR_NOMEM", name, nomem);
    CHECK(q.gc.pending.empty() && !q.gc.leader && !q.gc.lingering, "%s: queue not idle at the end", name);
    std::printf("%s: %zu calls in %zu batches (largest %zu), %zu threw, %d calls FTHE_ERR_NOMEM\n", name, calls,
                q.batches.load(), q.largest.load(), q.thrown_batches.load(), nomem);
}

// A lone caller never lingers: with a 2 s linger, 50 sequential calls take far less than one linger.
int lone_caller() {
    setenv("FTHE_LINGER_US", "2000000", 1);
    Queue q;
    const auto t0 = std::chrono::steady_clock::now();
    for (int j = 0; j < 50; j++) {
        Req r{(uint64_t)j, j % 3, false};
        CHECK(q.call(r) == FTHE_OK && r.out == result_of(r.in, r.key), "lone call %d", j);
    }
    const int64_t us = us_since(t0);
    CHECK(linger_us() == 2000000, "FTHE_LINGER_US not read: %d", linger_us());
    CHECK(us < 1000000, "50 lone calls took %lld us: a lone caller lingered", (long long)us);
    CHECK(q.batches == 50, "%zu batches for 50 lone calls", q.batches.load());
    std::printf("lone caller: 50 calls in %lld us with FTHE_LINGER_US=2000000\n", (long long)us);
    return failures ? 1 : 0;
}

}  // namespace

int main() {
    // FTHE_LINGER_US is read once per process: the lone-caller check sets its own in a child, forked before any thread
    std::fflush(nullptr);
    const pid_t child = fork();
    if (child == 0) { const int rc = lone_caller(); std::fflush(nullptr); _exit(rc); }
    int st = 0;
    CHECK(child > 0 && waitpid(child, &st, 0) == child && WIFEXITED(st) && WEXITSTATUS(st) == 0,
          "lone-caller child: status %d", st);

    // no thread may block: the watchdog aborts the run after 60 s
    std::mutex wd_mu; std::condition_variable wd_cv; bool finished = false;
    std::thread watchdog([&] {
        std::unique_lock<std::mutex> lk(wd_mu);
        if (!wd_cv.wait_for(lk, std::chrono::seconds(60), [&] { return finished; })) {
            std::fprintf(stderr, "FAIL: a caller blocked (60 s)\n");
            std::abort();
        }
    });

    check_grouping();
    {   // two queues driven at once, one leader at a time in each; a chosen call of queue a makes its batch throw
        Queue a, b;
        std::vector<std::thread> ths;
        std::atomic<int> nomem_a{0}, nomem_b{0};
        drive(a, ths, 5, 100, nomem_a);
        drive(b, ths, -1, -1, nomem_b);
        for (auto &t : ths) t.join();
        check_queue("queue a", a, (size_t)kThreads * kCalls, 1, nomem_a);
        check_queue("queue b", b, (size_t)kThreads * kCalls, 0, nomem_b);
        Req after{7, 1, false};                          // the queue that threw still serves
        CHECK(a.call(after) == FTHE_OK && after.out == result_of(7, 1), "call after the throw: rc %d", after.rc);
    }
    {   // two queues share no lock: each runner waits until the other is in flight too
        Queue a, b;
        a.other_entered = &b.entered; b.other_entered = &a.entered;
        Req ra{1, 0, false}, rb{2, 0, false};
        std::thread ta([&] { CHECK(a.call(ra) == FTHE_OK, "queue a: rc %d", ra.rc); });
        std::thread tb([&] { CHECK(b.call(rb) == FTHE_OK, "queue b: rc %d", rb.rc); });
        ta.join(); tb.join();
        CHECK(a.met && b.met, "the runners of two queues were never in flight together");
        std::printf("two queues in flight together: %s\n", a.met && b.met ? "yes" : "no");
    }

    { std::lock_guard<std::mutex> g(wd_mu); finished = true; }
    wd_cv.notify_all();
    watchdog.join();
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("group commit OK (FTHE_LINGER_US=%d)\n", linger_us());
    return 0;
}
