// oip_rankguard.hpp -- how the rank threads of the N-GPU host (oip_multigpu.hpp) meet, fail and give up together.
// No GPU or RCCL types in here: tests/test_cli_cpu.py builds it with ThreadSanitizer on the CPU.
//
//   HostBarrier   the ranks' meeting point; abort() releases everybody (wait() returns false from then on).
//   CommGuard     the communicators.  Every use of a communicator -- a single call or a whole ncclGroupStart..End
//                 sequence -- runs inside use().  abort_all() sets the aborted flag first, so every later use() throws
//                 PeerFailed, then runs the abort function on every communicator exactly once WITHOUT waiting for the calls in
//                 flight: a peer may sit inside use() in a call that blocks until the failed rank arrives (a connection
//                 handshake), and the abort is what releases it (the earlier guard took a lock exclusively there and
//                 could wait for ever).  The abort function therefore only wakes and fails calls; it frees nothing.  The owner
//                 frees the communicators after the rank threads have joined, so no call can touch a freed one.
//   FirstFailure  which rank gave up first, and why: the others' exceptions are consequences (PeerFailed, or a call that the
//                 abort made fail), whatever their rank index.
#pragma once

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <exception>
#include <stdexcept>
#include <vector>

namespace OIPGPU {

struct PeerFailed : public std::runtime_error {
    PeerFailed() : std::runtime_error("another GPU's step failed") {}
};

struct HostBarrier {
    std::mutex mu;
    std::condition_variable cv;
    int n, waiting = 0;
    unsigned long gen = 0;
    bool aborted = false;
    explicit HostBarrier(int n_) : n(n_) {}
    bool wait()                 // false: a rank has given up (abort()), nobody waits any longer
    {
        std::unique_lock<std::mutex> lk(mu);
        if (aborted) return false;
        const unsigned long g = gen;
        if (++waiting == n) { waiting = 0; ++gen; cv.notify_all(); }
        else cv.wait(lk, [&] { return gen != g || aborted; });
        return !aborted;
    }
    void abort()
    {
        std::unique_lock<std::mutex> lk(mu);
        aborted = true;
        cv.notify_all();
    }
};

template <typename Comm> class CommGuard {
public:
    explicit CommGuard(int n) : comm((size_t)n, Comm()) {}
    std::vector<Comm> comm;                     // filled by the owner before the rank threads start, freed by it after they joined
    // f(communicator of rank r); PeerFailed once the communicators have been aborted
    template <typename F> void use(int r, F f)
    {
        if (mAborted.load()) throw PeerFailed();
        f(comm[(size_t)r]);
    }
    // abort_one(communicator) for every communicator, once; it runs beside the calls in flight and must free nothing
    template <typename A> void abort_all(A abort_one)
    {
        if (mAborted.exchange(true)) return;
        for (auto &c : comm) abort_one(c);
    }
    bool aborted() const { return mAborted.load(); }

private:
    std::atomic<bool> mAborted{false};
};

class FirstFailure {
public:
    explicit FirstFailure(int n) : mEx((size_t)n) {}
    // rank r's thread gives up with exception e; call it before anything that makes the peers fail (barrier abort, communicator abort)
    void note(int r, std::exception_ptr e)
    {
        mEx[(size_t)r] = e;
        int none = -1;
        mFirst.compare_exchange_strong(none, r);
    }
    bool any() const { return mFirst.load() >= 0; }
    int rank() const { return mFirst.load(); }
    void rethrow() const                        // after the rank threads have joined
    {
        if (any()) std::rethrow_exception(mEx[(size_t)rank()]);
    }

private:
    std::vector<std::exception_ptr> mEx;
    std::atomic<int> mFirst{-1};
};

}  // namespace OIPGPU
