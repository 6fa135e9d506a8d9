// loopcomm_test.cpp -- the loopback communicator of the N-GPU host (csrc/oip_loopcomm.hpp) on the CPU, under ThreadSanitizer and
// ASan + UBSan: host memory, and a fake stream that runs every copy at once (an "event" is a heap token, so a leaked, doubly
// released or never-recorded one is a sanitizer report).  N rank threads drive it the way oip_multigpu.hpp does:
//   plans      random exchange plans, 2-4 ranks, many rounds: every rank iterates the same global list of groups (post_pieces),
//              skips the groups it has no part in; some groups go one way only; a halo-style group and an all-gather follow;
//              every received buffer holds the sender's bytes and the accounting equals the plan's sums;
//   mismatch   a matched send / receive of different sizes: both ranks get the error, neither blocks;
//   abort      a rank aborts while its peers sit inside a blocking group end, a blocking single send and an all-gather;
//   deadline   a rank whose peer never arrives gets the timed-out error (send, recv and allgather).
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>

#include "oip_loopcomm.hpp"

using namespace OIPGPU;
using Clock = std::chrono::steady_clock;

static std::atomic<long> g_events{0}, g_copies{0};

static LoopDeviceOps fake_ops()
{
    LoopDeviceOps o;
    o.record = [](void *) -> void * { ++g_events; return new int(1); };
    o.wait = [](void *, void *e) { return e && *(int *)e == 1; };                  // only ever an event that was recorded
    o.copy = [](void *d, const void *s, size_t n, void *) { memcpy(d, s, n); ++g_copies; return true; };
    o.release = [](void *e) { --g_events; delete (int *)e; };
    return o;
}

static double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

struct Transfer { int src, dst; size_t bytes; };
static uint8_t pattern(int round, int group, int k, int src, size_t i) { return (uint8_t)(round * 131 + group * 31 + k * 17 + src * 7 + i * 3 + (i >> 8)); }

// one round's plan, the same on every rank (same seed)
struct RoundPlan {
    std::vector<std::vector<Transfer>> groups;      // the last one is the halo-style group
    size_t gather_bytes;
    RoundPlan(int N, int round)
    {
        std::mt19937 rng((unsigned)(N * 100003 + round));
        auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
        const int ng = 1 + pick(6);
        for (int g = 0; g < ng; ++g) {
            std::vector<Transfer> t;
            const int nt = pick(6);                 // (an empty group is skipped by everybody)
            const bool one_way = pick(3) == 0;
            const int a = pick(N), b = (a + 1 + pick(N - 1)) % N;
            for (int k = 0; k < nt; ++k) {
                int s = pick(N), d = (s + 1 + pick(N - 1)) % N;
                if (one_way) { s = a; d = b; }
                t.push_back(Transfer{s, d, (size_t)(1 + pick(3000))});
            }
            groups.push_back(t);
        }
        std::vector<Transfer> halo;                 // whole "lines" to the neighbours, as exchange_lines sends them
        for (int r = 0; r < N; ++r) {
            if (r > 0 && pick(4)) halo.push_back(Transfer{r, r - 1, (size_t)(64 * (1 + pick(8)))});
            if (r + 1 < N && pick(4)) halo.push_back(Transfer{r, r + 1, (size_t)(64 * (1 + pick(8)))});
        }
        groups.push_back(halo);
        gather_bytes = (size_t)(8 * (1 + pick(12)));
    }
};

static int case_plans(int N, int rounds)
{
    std::vector<LoopComm *> comm = loop_init_all(N, fake_ops(), 20.0);
    std::atomic<int> bad{0};
    std::vector<LoopStats> want((size_t)N);
    for (int round = 0; round < rounds; ++round) {
        RoundPlan p(N, round);
        for (auto &g : p.groups)
            for (auto &t : g) {
                ++want[(size_t)t.src].sends; want[(size_t)t.src].send_bytes += (long)t.bytes;
                ++want[(size_t)t.dst].recvs; want[(size_t)t.dst].recv_bytes += (long)t.bytes;
            }
        for (int r = 0; r < N; ++r) { ++want[(size_t)r].gathers; want[(size_t)r].gather_bytes += (long)p.gather_bytes; }
    }
    std::vector<std::thread> th;
    for (int r = 0; r < N; ++r)
        th.emplace_back([&, r] {
            void *stream = &comm[(size_t)r];
            auto fail = [&](const char *what, int round) { printf("plans N=%d rank %d round %d: %s: %s\n", N, r, round, what, loop_last_error()); ++bad; };
            for (int round = 0; round < rounds; ++round) {
                RoundPlan p(N, round);
                for (size_t g = 0; g < p.groups.size(); ++g) {
                    const auto &ts = p.groups[g];
                    bool any = false;
                    for (auto &t : ts) any = any || t.src == r || t.dst == r;
                    if (!any) continue;
                    std::vector<std::vector<uint8_t>> sbuf(ts.size()), rbuf(ts.size());
                    if (loop_group_start()) return fail("group start", round);
                    if (loop_group_start()) return fail("nested group start", round);       // groups nest per thread
                    for (size_t k = 0; k < ts.size(); ++k)
                        if (ts[k].src == r) {
                            sbuf[k].resize(ts[k].bytes);
                            for (size_t i = 0; i < ts[k].bytes; ++i) sbuf[k][i] = pattern(round, (int)g, (int)k, r, i);
                            if (loop_send(comm[(size_t)r], sbuf[k].data(), ts[k].bytes, ts[k].dst, stream)) return fail("send", round);
                        }
                    if (loop_group_end()) return fail("inner group end", round);
                    for (size_t k = 0; k < ts.size(); ++k)
                        if (ts[k].dst == r) {
                            rbuf[k].assign(ts[k].bytes, 0);
                            if (loop_recv(comm[(size_t)r], rbuf[k].data(), ts[k].bytes, ts[k].src, stream)) return fail("recv", round);
                        }
                    if (loop_group_end()) return fail("group end", round);
                    for (size_t k = 0; k < ts.size(); ++k)
                        if (ts[k].dst == r)
                            for (size_t i = 0; i < ts[k].bytes; ++i)
                                if (rbuf[k][i] != pattern(round, (int)g, (int)k, ts[k].src, i)) return fail("received bytes differ", round);
                }
                std::vector<uint8_t> mine(p.gather_bytes), all(p.gather_bytes * (size_t)N, 0);
                for (size_t i = 0; i < p.gather_bytes; ++i) mine[i] = pattern(round, 99, 0, r, i);
                if (loop_allgather(comm[(size_t)r], mine.data(), all.data(), p.gather_bytes, stream)) return fail("allgather", round);
                for (int q = 0; q < N; ++q)
                    for (size_t i = 0; i < p.gather_bytes; ++i)
                        if (all[(size_t)q * p.gather_bytes + i] != pattern(round, 99, 0, q, i)) return fail("gathered bytes differ", round);
            }
        });
    for (auto &t : th) t.join();
    for (int r = 0; r < N; ++r) {
        const LoopStats s = loop_stats(comm[(size_t)r]), &w = want[(size_t)r];
        if (s.sends != w.sends || s.send_bytes != w.send_bytes || s.recvs != w.recvs || s.recv_bytes != w.recv_bytes || s.gathers != w.gathers ||
            s.gather_bytes != w.gather_bytes) {
            printf("plans N=%d rank %d: accounting %ld/%ld %ld/%ld %ld/%ld, plan %ld/%ld %ld/%ld %ld/%ld\n", N, r, s.sends, s.send_bytes, s.recvs,
                   s.recv_bytes, s.gathers, s.gather_bytes, w.sends, w.send_bytes, w.recvs, w.recv_bytes, w.gathers, w.gather_bytes);
            ++bad;
        }
    }
    for (auto c : comm) loop_destroy(c);
    if (g_events != 0) { printf("plans N=%d: %ld events not released\n", N, g_events.load()); ++bad; }
    return bad;
}

static int case_mismatch()
{
    std::vector<LoopComm *> comm = loop_init_all(2, fake_ops(), 20.0);
    std::string err[2];
    std::vector<uint8_t> a(100, 1), b(120, 0);
    const auto t0 = Clock::now();
    std::thread t1([&] { if (loop_send(comm[0], a.data(), 100, 1, nullptr)) err[0] = loop_last_error(); });
    std::thread t2([&] {
        loop_group_start();
        loop_recv(comm[1], b.data(), 120, 0, nullptr);
        if (loop_group_end()) err[1] = loop_last_error();
    });
    t1.join(); t2.join();
    const double s = seconds_since(t0);
    for (auto c : comm) loop_destroy(c);
    const std::string want = "loopback: rank 0 sends 100 bytes to rank 1, which receives 120 bytes from it";
    if (err[0] != want || err[1] != want || s > 5.0) {
        printf("mismatch: [%s] [%s] after %.2f s\n", err[0].c_str(), err[1].c_str(), s);
        return 1;
    }
    return 0;
}

static int case_abort()
{
    std::vector<LoopComm *> comm = loop_init_all(4, fake_ops(), 30.0);
    std::string err[3];
    std::atomic<int> inside{0}, bad{0};
    std::vector<uint8_t> buf(3 * 256, 0), all(4 * 64, 0);
    const auto t0 = Clock::now();
    std::vector<std::thread> th;
    th.emplace_back([&] {                               // inside a blocking group end: rank 3 never posts
        loop_group_start();
        loop_recv(comm[0], buf.data(), 256, 3, nullptr);
        loop_send(comm[0], buf.data() + 256, 64, 3, nullptr);
        ++inside;
        if (loop_group_end()) err[0] = loop_last_error();
    });
    th.emplace_back([&] { ++inside; if (loop_allgather(comm[1], buf.data() + 512, all.data(), 64, nullptr)) err[1] = loop_last_error(); });
    th.emplace_back([&] { ++inside; if (loop_send(comm[2], buf.data() + 512, 64, 3, nullptr)) err[2] = loop_last_error(); });
    th.emplace_back([&] {
        while (inside < 3) std::this_thread::yield();
        std::this_thread::sleep_for(std::chrono::milliseconds(100));      // (let them reach their waits; the outcome does not depend on it)
        loop_abort(comm[3]);
    });
    for (auto &t : th) t.join();
    const double s = seconds_since(t0);
    for (int r = 0; r < 3; ++r)
        if (err[r] != "loopback communicator aborted") { printf("abort: rank %d got [%s]\n", r, err[r].c_str()); ++bad; }
    if (s > 5.0) { printf("abort: the waiters took %.2f s\n", s); ++bad; }
    for (int r = 0; r < 4; ++r) {                       // every later call on any communicator fails, at once
        std::thread t([&, r] {
            loop_group_start();
            const int rc = loop_recv(comm[(size_t)r], buf.data(), 8, (r + 1) % 4, nullptr);
            if (!rc || std::string(loop_last_error()) != "loopback communicator aborted") { printf("abort: a later call on rank %d went through\n", r); ++bad; }
            if (!loop_allgather(comm[(size_t)r], buf.data(), all.data(), 8, nullptr)) { printf("abort: a later allgather on rank %d went through\n", r); ++bad; }
        });
        t.join();
    }
    for (auto c : comm) loop_destroy(c);                // freed only now: the rank threads have joined
    if (g_events != 0) { printf("abort: %ld events not released\n", g_events.load()); ++bad; }
    return bad;
}

static int case_deadline()
{
    int bad = 0;
    struct { const char *what; int n; std::function<int(LoopComm *, uint8_t *)> call; std::string want; } cases[] = {
        {"recv", 2, [](LoopComm *c, uint8_t *b) { return loop_recv(c, b, 64, 1, nullptr); }, "loopback rendezvous timed out: rank 0 waiting for rank 1 (recv, 64 bytes)"},
        {"send", 3, [](LoopComm *c, uint8_t *b) { loop_group_start(); loop_send(c, b, 48, 2, nullptr); return loop_group_end(); },
         "loopback rendezvous timed out: rank 0 waiting for rank 2 (send, 48 bytes)"},
        {"allgather", 2, [](LoopComm *c, uint8_t *b) { return loop_allgather(c, b, b + 16, 16, nullptr); },
         "loopback rendezvous timed out: rank 0 waiting for rank 1 (allgather, 16 bytes)"},
    };
    for (auto &k : cases) {
        std::vector<LoopComm *> comm = loop_init_all(k.n, fake_ops(), 0.2);
        uint8_t buf[64] = {0};
        const auto t0 = Clock::now();
        const int rc = k.call(comm[0], buf);
        const double s = seconds_since(t0);
        if (!rc || k.want != loop_last_error() || s < 0.19 || s > 5.0) { printf("deadline %s: rc %d [%s] after %.2f s\n", k.what, rc, loop_last_error(), s); ++bad; }
        for (auto c : comm) loop_destroy(c);
    }
    if (g_events != 0) { printf("deadline: %ld events not released\n", g_events.load()); ++bad; }
    return bad;
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    int bad = 0, cases = 0;
    for (int N = 2; N <= 4; ++N, ++cases) bad += case_plans(N, rounds);
    bad += case_mismatch(); ++cases;
    bad += case_abort(); ++cases;
    bad += case_deadline(); ++cases;
    printf("%d cases, %d rounds per plan case, %ld copies, %d bad\n", cases, rounds, g_copies.load(), bad);
    return bad ? 1 : 0;
}
