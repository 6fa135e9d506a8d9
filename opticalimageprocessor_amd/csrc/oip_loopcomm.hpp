// oip_loopcomm.hpp -- a loopback communicator: the N ranks of the N-GPU host (oip_multigpu.hpp) meeting inside one process.
// No GPU or RCCL types in here (as oip_rankguard.hpp): tests/cpp/loopcomm_test.cpp drives it on the CPU with host memory under
// ThreadSanitizer and ASan + UBSan; oip_multigpu.hpp binds it into its RcclApi table for OIP_COMM=loopback, where every rank
// uses one GPU.  It is a TEST device: it proves the host's ordering and addressing, not RCCL's behaviour or any link rate.
//
// Semantics, as far as the host uses NCCL:
//   send / recv      between a pair (src, dst) match in posting order; a matched pair that disagrees in byte count is an error
//                    on both ranks that names both ranks and both sizes (RCCL would not notice; the plans are symmetric);
//   group            group_start / group_end nest per thread.  The outermost group_end BLOCKS: it posts all of its operations
//                    first, without blocking, then waits until each is matched and its device work is enqueued (RCCL's blocking
//                    connection handshake); outside a group the single call blocks instead;
//   allgather        rank q's bytes land at recv + q * bytes;
//   abort            wakes every waiter; every later call on any communicator of the world fails;
//   deadline         every host-side wait ends after OIP_LOOPBACK_TIMEOUT_S seconds (default 30) with
//                    "loopback rendezvous timed out: rank r waiting for rank q (send|recv|allgather, k bytes)".
// Device work of a matched pair (LoopDeviceOps: HIP events and copies in the host, plain memcpy in the CPU test):
//   the sender records an event on its stream when it posts; the receiver's stream waits for that event, runs one copy and
//   records a "done" event; the sender's stream waits for that one, so the sender may reuse its buffer.  Every rank's thread
//   touches its own stream only.  No stream is ever made to wait for an event that has not been recorded yet and nothing on the
//   device waits for the host: a protocol mistake can only block host threads, and those have the deadline.
#pragma once

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace OIPGPU {

struct LoopDeviceOps {
    std::function<void *(void *stream)> record;                                             // a new event, recorded on stream; nullptr: failed
    std::function<bool(void *stream, void *event)> wait;                                    // stream waits for a recorded event
    std::function<bool(void *dst, const void *src, size_t bytes, void *stream)> copy;       // one copy on stream
    std::function<void(void *event)> release;
};

struct LoopStats {
    long sends = 0, send_bytes = 0, recvs = 0, recv_bytes = 0, gathers = 0, gather_bytes = 0;
};

class LoopWorld;
struct LoopGroup;
struct LoopComm {
    LoopWorld *world;
    int rank;
};

class LoopWorld {
public:
    LoopWorld(int n, LoopDeviceOps ops_, double timeout_s = -1.0)
        : N(n), ops(std::move(ops_)), chan((size_t)n * n), send_seq((size_t)n * n, 0), recv_seq((size_t)n * n, 0), gather_seq((size_t)n, 0),
          stats_((size_t)n), comms((size_t)n), alive(n)
    {
        if (timeout_s <= 0.0) {
            const char *e = getenv("OIP_LOOPBACK_TIMEOUT_S");
            timeout_s = e ? atof(e) : 30.0;
            if (!(timeout_s > 0.0)) timeout_s = 30.0;
        }
        timeout = std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>(timeout_s));
        for (int r = 0; r < n; ++r) comms[(size_t)r] = LoopComm{this, r};
    }
    ~LoopWorld()
    {
        for (void *e : events) ops.release(e);
    }
    LoopComm *comm(int r) { return &comms[(size_t)r]; }
    LoopStats stats(int r)
    {
        std::lock_guard<std::mutex> lk(mu);
        return stats_[(size_t)r];
    }
    bool is_aborted()
    {
        std::lock_guard<std::mutex> lk(mu);
        return aborted;
    }
    void abort()
    {
        std::lock_guard<std::mutex> lk(mu);
        aborted = true;
        cv.notify_all();
    }
    bool release_one()              // a communicator is destroyed; true: it was the last one, the caller deletes the world
    {
        std::lock_guard<std::mutex> lk(mu);
        return --alive == 0;
    }

    const int N;

private:
    friend struct LoopGroup;
    struct Xfer {                   // one send and the receive it matches
        bool send_posted = false, recv_posted = false;
        const void *src = nullptr;
        size_t send_bytes = 0, recv_bytes = 0;
        void *ready = nullptr, *done = nullptr;          // the sender's event, the receiver's event
    };
    struct Gather {
        std::vector<const void *> send;
        std::vector<size_t> bytes;
        std::vector<void *> ready, done;
        int posted = 0, copied = 0;
        explicit Gather(int n) : send((size_t)n, nullptr), bytes((size_t)n, 0), ready((size_t)n, nullptr), done((size_t)n, nullptr) {}
    };
    std::shared_ptr<Xfer> xfer_of(int src, int dst, bool sender)        // (mu held) the k-th transfer of the pair, k in posting order
    {
        const size_t c = (size_t)src * N + dst;
        const long k = sender ? send_seq[c]++ : recv_seq[c]++;
        auto &slot = chan[c][k];
        if (!slot) slot = std::make_shared<Xfer>();
        std::shared_ptr<Xfer> x = slot;
        if (k < std::min(send_seq[c], recv_seq[c])) chan[c].erase(k);   // both sides hold it now
        return x;
    }
    std::shared_ptr<Gather> gather_of(int r)                            // (mu held)
    {
        const long k = gather_seq[(size_t)r]++;
        auto &slot = gathers[k];
        if (!slot) slot = std::make_shared<Gather>(N);
        std::shared_ptr<Gather> g = slot;
        if (g->posted + 1 == N) gathers.erase(k);
        return g;
    }

    LoopDeviceOps ops;
    std::mutex mu;
    std::condition_variable cv;
    bool aborted = false;
    std::chrono::steady_clock::duration timeout;
    std::vector<std::map<long, std::shared_ptr<Xfer>>> chan;            // [src * N + dst]
    std::vector<long> send_seq, recv_seq, gather_seq;
    std::map<long, std::shared_ptr<Gather>> gathers;
    std::vector<LoopStats> stats_;
    std::vector<void *> events;                                         // released with the world: after every stream has been drained
    std::vector<LoopComm> comms;
    int alive;
};

// the calling thread's open group and its last error
struct LoopGroup {
    enum Kind { Send, Recv, AllGather };
    struct Op {
        Kind kind;
        LoopComm *c;
        int peer;
        const void *sbuf;
        void *rbuf;
        size_t bytes;
        void *stream;
        std::shared_ptr<LoopWorld::Xfer> x;
        std::shared_ptr<LoopWorld::Gather> g;
        void *ready = nullptr;                      // this rank's "bytes are ready" event of a send or an all-gather
        int phase = 0;
        bool finished = false;
    };
    int depth = 0;
    std::vector<Op> ops;
    std::string error;

    static LoopGroup &mine()
    {
        static thread_local LoopGroup g;
        return g;
    }
    int fail(const std::string &m)
    {
        error = m;
        depth = 0;
        ops.clear();
        return 1;
    }
    static const char *name(Kind k) { return k == Send ? "send" : k == Recv ? "recv" : "allgather"; }

    int add(Op op)
    {
        LoopWorld *w = op.c->world;
        if (w->is_aborted()) return fail("loopback communicator aborted");
        if (op.kind != AllGather && (op.peer < 0 || op.peer >= w->N || op.peer == op.c->rank))
            return fail("loopback: rank " + std::to_string(op.c->rank) + " names peer " + std::to_string(op.peer));
        if (!ops.empty() && ops[0].c->world != w) return fail("loopback: one group, two worlds");
        ops.push_back(op);
        return depth > 0 ? 0 : run();
    }
    int start()
    {
        ++depth;
        return 0;
    }
    int end()
    {
        if (depth <= 0) return fail("loopback: group end without a group start");
        if (--depth > 0 || ops.empty()) return 0;
        return run();
    }

private:
    // post everything, then wait until every operation is matched and its device work enqueued
    int run()
    {
        LoopWorld *w = ops[0].c->world;
        const LoopDeviceOps &dev = w->ops;
        // the events that say "this rank's bytes are ready" are recorded before they are published
        for (Op &op : ops)
            if (op.kind != Recv && !(op.ready = dev.record(op.stream))) return fail("loopback: event record failed");
        std::unique_lock<std::mutex> lk(w->mu);
        for (Op &op : ops) {
            const int r = op.c->rank;
            LoopStats &s = w->stats_[(size_t)r];
            if (op.kind == Send) {
                op.x = w->xfer_of(r, op.peer, true);
                op.x->send_posted = true; op.x->src = op.sbuf; op.x->send_bytes = op.bytes; op.x->ready = op.ready;
                w->events.push_back(op.ready);
                ++s.sends; s.send_bytes += (long)op.bytes;
            } else if (op.kind == Recv) {
                op.x = w->xfer_of(op.peer, r, false);
                op.x->recv_posted = true; op.x->recv_bytes = op.bytes;
                ++s.recvs; s.recv_bytes += (long)op.bytes;
            } else {
                op.g = w->gather_of(r);
                op.g->send[(size_t)r] = op.sbuf; op.g->bytes[(size_t)r] = op.bytes; op.g->ready[(size_t)r] = op.ready;
                w->events.push_back(op.ready);
                ++op.g->posted;
                ++s.gathers; s.gather_bytes += (long)op.bytes;
            }
        }
        w->cv.notify_all();
        const auto deadline = std::chrono::steady_clock::now() + w->timeout;
        for (;;) {
            if (w->aborted) return fail_unlocked(lk, "loopback communicator aborted");
            bool all = true, progressed = false;
            const Op *blocked = nullptr;
            int blocked_on = -1;
            for (Op &op : ops) {
                if (op.finished) continue;
                std::string err;
                int waits_for = -1;
                const bool moved = op.kind == AllGather ? step_gather(w, lk, op, &err, &waits_for) : step_xfer(w, lk, op, &err);
                if (!err.empty()) return fail_unlocked(lk, err);
                progressed = progressed || moved;
                if (!op.finished) {
                    all = false;
                    if (!moved && !blocked) { blocked = &op; blocked_on = op.kind == AllGather ? waits_for : op.peer; }
                }
            }
            if (all) break;
            if (progressed) continue;
            const auto now = std::chrono::steady_clock::now();
            if (now >= deadline)
                return fail_unlocked(lk, "loopback rendezvous timed out: rank " + std::to_string(blocked->c->rank) + " waiting for rank " +
                                             std::to_string(blocked_on) + " (" + name(blocked->kind) + ", " + std::to_string(blocked->bytes) + " bytes)");
            // (the deadline is the steady clock's; the wait itself is given a system_clock time so that it is a
            // pthread_cond_timedwait, which ThreadSanitizer understands -- it does not follow pthread_cond_clockwait)
            w->cv.wait_until(lk, std::chrono::system_clock::now() + (deadline - now));
        }
        lk.unlock();
        ops.clear();
        return 0;
    }
    int fail_unlocked(std::unique_lock<std::mutex> &lk, const std::string &m)
    {
        lk.unlock();
        return fail(m);
    }
    static std::string mismatch(int src, int dst, size_t sb, size_t rb)
    {
        return "loopback: rank " + std::to_string(src) + " sends " + std::to_string(sb) + " bytes to rank " + std::to_string(dst) +
               ", which receives " + std::to_string(rb) + " bytes from it";
    }
    // one step of a send or a receive (mu held on entry and on return; released around the device calls).  true: it moved
    bool step_xfer(LoopWorld *w, std::unique_lock<std::mutex> &lk, Op &op, std::string *err)
    {
        LoopWorld::Xfer &x = *op.x;
        const int r = op.c->rank;
        if (!x.send_posted || !x.recv_posted) return false;
        if (x.send_bytes != x.recv_bytes) {
            *err = op.kind == Send ? mismatch(r, op.peer, x.send_bytes, x.recv_bytes) : mismatch(op.peer, r, x.send_bytes, x.recv_bytes);
            return false;
        }
        if (op.kind == Send) {
            if (!x.done) return false;
            void *done = x.done;
            lk.unlock();
            const bool ok = w->ops.wait(op.stream, done);              // the buffer is free again behind this point of the stream
            lk.lock();
            if (!ok) { *err = "loopback: stream wait failed"; return false; }
            op.finished = true;
            return true;
        }
        const void *src = x.src;
        void *ready = x.ready;
        lk.unlock();
        void *done = nullptr;
        const bool ok = w->ops.wait(op.stream, ready) && w->ops.copy(op.rbuf, src, op.bytes, op.stream) && (done = w->ops.record(op.stream));
        lk.lock();
        if (!ok) { *err = "loopback: copy of " + std::to_string(op.bytes) + " bytes from rank " + std::to_string(op.peer) + " failed"; return false; }
        x.done = done;
        w->events.push_back(done);
        w->cv.notify_all();
        op.finished = true;
        return true;
    }
    bool step_gather(LoopWorld *w, std::unique_lock<std::mutex> &lk, Op &op, std::string *err, int *waits_for)
    {
        LoopWorld::Gather &g = *op.g;
        const int r = op.c->rank, N = w->N;
        if (op.phase == 0) {
            if (g.posted < N) {
                for (int q = 0; q < N; ++q) if (!g.ready[(size_t)q]) { *waits_for = q; break; }
                return false;
            }
            for (int q = 0; q < N; ++q)
                if (g.bytes[(size_t)q] != op.bytes) {
                    *err = "loopback: allgather of " + std::to_string(op.bytes) + " bytes on rank " + std::to_string(r) + ", of " +
                           std::to_string(g.bytes[(size_t)q]) + " bytes on rank " + std::to_string(q);
                    return false;
                }
            lk.unlock();
            bool ok = true;
            for (int q = 0; q < N && ok; ++q)
                ok = w->ops.wait(op.stream, g.ready[(size_t)q]) &&
                     w->ops.copy((char *)op.rbuf + (size_t)q * op.bytes, g.send[(size_t)q], op.bytes, op.stream);
            void *done = ok ? w->ops.record(op.stream) : nullptr;
            lk.lock();
            if (!done) { *err = "loopback: allgather copy failed"; return false; }
            g.done[(size_t)r] = done;
            w->events.push_back(done);
            ++g.copied;
            w->cv.notify_all();
            op.phase = 1;
            return true;
        }
        if (g.copied < N) {
            for (int q = 0; q < N; ++q) if (!g.done[(size_t)q]) { *waits_for = q; break; }
            return false;
        }
        lk.unlock();
        bool ok = true;
        for (int q = 0; q < N && ok; ++q) if (q != r) ok = w->ops.wait(op.stream, g.done[(size_t)q]);       // every peer has read this rank's bytes
        lk.lock();
        if (!ok) { *err = "loopback: stream wait failed"; return false; }
        op.finished = true;
        return true;
    }
};

// ---- the calls (0: done; otherwise loop_last_error() tells why, on the calling thread) ---------------------------------------
inline std::vector<LoopComm *> loop_init_all(int n, LoopDeviceOps ops, double timeout_s = -1.0)
{
    LoopWorld *w = new LoopWorld(n, std::move(ops), timeout_s);
    std::vector<LoopComm *> v;
    for (int r = 0; r < n; ++r) v.push_back(w->comm(r));
    return v;
}
inline int loop_group_start() { return LoopGroup::mine().start(); }
inline int loop_group_end() { return LoopGroup::mine().end(); }
inline int loop_send(LoopComm *c, const void *buf, size_t bytes, int peer, void *stream)
{
    return LoopGroup::mine().add(LoopGroup::Op{LoopGroup::Send, c, peer, buf, nullptr, bytes, stream, nullptr, nullptr});
}
inline int loop_recv(LoopComm *c, void *buf, size_t bytes, int peer, void *stream)
{
    return LoopGroup::mine().add(LoopGroup::Op{LoopGroup::Recv, c, peer, nullptr, buf, bytes, stream, nullptr, nullptr});
}
inline int loop_allgather(LoopComm *c, const void *send, void *recv, size_t bytes, void *stream)
{
    return LoopGroup::mine().add(LoopGroup::Op{LoopGroup::AllGather, c, -1, send, recv, bytes, stream, nullptr, nullptr});
}
inline int loop_abort(LoopComm *c)                  // wakes every waiter of the world; frees nothing
{
    c->world->abort();
    return 0;
}
inline int loop_destroy(LoopComm *c)                // after the rank threads are done with it; the last one frees the world
{
    LoopWorld *w = c->world;
    if (w->release_one()) delete w;
    return 0;
}
inline LoopStats loop_stats(LoopComm *c) { return c->world->stats(c->rank); }
inline const char *loop_last_error() { return LoopGroup::mine().error.c_str(); }

}  // namespace OIPGPU
