// Group commit for the key's shared calls (fthe_decrypt_shared, fthe_encrypt_shared, fthe_add_shared /
// fthe_scalar_mul_u64_shared): the queue protocol, once.  Standard library only, so the one piece of lock and
// condition-variable code in the library builds and runs without a GPU (tools/group_commit_test.cpp).
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/fthe.h"

// Group commit with a linger.  The callers of a finished batch come back one at a time (each wakes from
// notify_all, re-takes the mutex, returns, issues its next call), so a new leader that took the queue at
// once would run a batch of one and leave the others to the round trip after: FedTree's OpenMP loops of
// single-element calls (hist_tree_builder.cpp:574-591 through GHPair's operators; decrypt_gh per node,
// FLtrainer.cpp:758-764) ran two launches per round.  A new leader waits until as many requests are pending
// as there were callers in the previous round (its batch plus the requests that arrived while it ran), at
// most FTHE_LINGER_US (default 200 us; 0: off) or a quarter of the previous batch's duration if that is
// longer (a merged decrypt takes ~10 ms), the latter capped at kLingerCapUs so one huge batch (a bulk
// add_shared of millions of rows) cannot make the next leader wait for callers that never come back; a lone
// caller never waits.  Arrivals wake it when the count is reached.
static constexpr int64_t kLingerCapUs = 3000;
inline int linger_us() {
    static const int v = [] {
        const char *e = getenv("FTHE_LINGER_US");
        return e ? std::max(0, atoi(e)) : 200;
    }();
    return v;
}
inline int64_t us_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

// One queue.  Req carries `int rc` and `bool done`; submit() blocks until r has been part of a batch and returns
// its rc.  One caller at a time is leader: it runs everything pending (its own request included) through
// run_batch(const std::vector<Req *> &), which sets every rc, then hands leadership to a caller still waiting.
template <class Req>
struct GroupCommit {
    std::mutex mu;
    std::condition_variable cv;      // a batch is done, leadership is free
    std::condition_variable lcv;     // the lingering leader: enough requests are pending
    std::vector<Req *> pending;
    bool leader = false, lingering = false;
    size_t last = 0;                 // callers active in the previous round
    int64_t last_us = 0;             // the previous batch's duration

    void linger(std::unique_lock<std::mutex> &lk) {
        if (last <= 1 || pending.size() >= last || linger_us() <= 0) return;
        lingering = true;
        // a quarter of a long batch (decrypts), capped: one huge batch must not make the next lone caller wait long
        const int64_t bound = std::max<int64_t>(linger_us(), std::min<int64_t>(last_us / 4, kLingerCapUs));
        lcv.wait_for(lk, std::chrono::microseconds(bound), [&] { return pending.size() >= last; });
        lingering = false;
    }
    void arrived() {
        if (lingering && pending.size() >= last) lcv.notify_all();
    }

    // Nothing leaves by exception, and the leader always marks its batch done and hands over: a throw from
    // run_batch (allocation failures: staging vectors, copy threads) becomes FTHE_ERR_NOMEM for every request
    // of that batch; a caller whose request cannot be queued returns FTHE_ERR_NOMEM without blocking anyone.
    template <class Run>
    int submit(Req &r, Run &&run_batch) {
        std::unique_lock<std::mutex> lk(mu);
        try { pending.push_back(&r); } catch (...) { return FTHE_ERR_NOMEM; }
        arrived();
        for (;;) {
            if (r.done) return r.rc;
            if (!leader) {
                leader = true;
                linger(lk);
                std::vector<Req *> batch;
                batch.swap(pending);                     // includes r
                lk.unlock();
                const auto t_batch = std::chrono::steady_clock::now();
                try {
                    run_batch(static_cast<const std::vector<Req *> &>(batch));
                } catch (...) {
                    for (Req *q : batch) q->rc = FTHE_ERR_NOMEM;
                }
                const int64_t us = us_since(t_batch);
                lk.lock();
                last_us = us;
                for (Req *q : batch) q->done = true;
                last = batch.size() + pending.size();    // callers active in this round
                leader = false;
                cv.notify_all();
                return r.rc;
            }
            cv.wait(lk);
        }
    }
};

// A batch split into groups that share one call: groups in the order their key first appears, the requests of a
// group in batch order.
template <class Req, class KeyOf>
auto group_by_key(const std::vector<Req *> &batch, KeyOf &&key_of) {
    using Key = decltype(key_of(*batch.front()));
    std::vector<std::pair<Key, std::vector<Req *>>> groups;
    for (Req *r : batch) {
        const Key key = key_of(*r);
        auto g = std::find_if(groups.begin(), groups.end(), [&](const auto &x) { return x.first == key; });
        if (g == groups.end()) g = groups.insert(g, {key, {}});
        g->second.push_back(r);
    }
    return groups;
}
