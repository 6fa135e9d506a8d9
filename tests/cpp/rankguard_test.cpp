// rankguard_test.cpp -- the failure protocol of the N-GPU host (csrc/oip_rankguard.hpp) on the CPU, under ThreadSanitizer:
// N rank threads pass the pre-exchange barrier and keep posting "RCCL calls" on fake communicators; one rank fails right
// behind the barrier and aborts them all (a peer used to be able to touch a communicator that ncclCommAbort had
// freed).  A fake communicator is a heap object: the owner deletes it after the rank threads have joined, a "call" reads and
// writes it -- so a use after it was freed is a use after free that TSan / ASan report, and the test checks the counters as well.
// Every second round the peers' call BLOCKS until the communicator is aborted, as a connection handshake with the failed rank
// does: a guard whose abort waits for the calls in flight never finishes such a round.  A blocked call that the
// abort released fails; that failure is a consequence, and the round must report the culprit's own message whatever its rank.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "oip_rankguard.hpp"

using namespace OIPGPU;

struct FakeComm {
    std::atomic<long> calls{0};
    bool alive = true;
    std::mutex mu;
    std::condition_variable cv;
    bool aborted = false;
    void abort()                                    // wakes and fails the calls; frees nothing
    {
        std::lock_guard<std::mutex> lk(mu);
        aborted = true;
        cv.notify_all();
    }
    bool blocking_call()                            // a handshake with a peer that never arrives: false once aborted
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return aborted; });
        return false;
    }
};

int main(int argc, char **argv)
{
    const int N = argc > 1 ? atoi(argv[1]) : 4, rounds = argc > 2 ? atoi(argv[2]) : 200;
    int bad = 0, blocking_rounds = 0;
    for (int round = 0; round < rounds; ++round) {
        const bool blocking = round % 2 == 1;
        blocking_rounds += blocking;
        HostBarrier bar(N);
        CommGuard<FakeComm *> comms(N);
        for (auto &c : comms.comm) c = new FakeComm();
        FirstFailure first(N);
        std::atomic<int> peer_failed{0}, own_failure{0}, used_after_free{0}, inside{0};
        const int culprit = round % N;
        auto give_up = [&](int r) {                 // Node::run's catch block
            first.note(r, std::current_exception());
            bar.abort();
            comms.abort_all([](FakeComm *c) { c->abort(); });
        };
        std::vector<std::thread> th;
        for (int r = 0; r < N; ++r)
            th.emplace_back([&, r] {
                try {
                    if (!bar.wait()) throw PeerFailed();                  // the barrier that precedes the exchange
                    if (r == culprit) {
                        // every fourth round the culprit fails only when all its peers sit inside their blocking call
                        if (blocking && round % 4 == 1) while (inside < N - 1) std::this_thread::yield();
                        else std::this_thread::sleep_for(std::chrono::microseconds(50 * (round % 7)));
                        throw std::runtime_error("injected on rank " + std::to_string(r));
                    }
                    for (int g = 0; g < 2000; ++g) {                      // groups of posted transfers
                        if (first.any()) throw PeerFailed();
                        comms.use(r, [&](FakeComm *c) {
                            if (!c->alive) ++used_after_free;             // (would also be a heap-use-after-free)
                            for (int k = 0; k < 8; ++k) ++c->calls;       // ncclGroupStart, sends, recvs, ncclGroupEnd
                            if (blocking && g == 3) {
                                ++inside;
                                if (!c->blocking_call()) {                // Node::nccl_ok: once the node has failed, a consequence
                                    if (first.any()) throw PeerFailed();
                                    throw std::runtime_error("ncclGroupEnd failed on rank " + std::to_string(r));
                                }
                            }
                        });
                    }
                    if (!bar.wait()) throw PeerFailed();                  // finish_pieces' meeting point
                } catch (const PeerFailed &) {
                    ++peer_failed;
                    give_up(r);
                } catch (const std::exception &) {
                    ++own_failure;
                    give_up(r);
                }
            });
        for (auto &t : th) t.join();
        std::string told;
        try { first.rethrow(); } catch (const std::exception &e) { told = e.what(); }
        for (auto &c : comms.comm) { if (!c->aborted) ++bad; c->alive = false; delete c; }     // freed by the owner, after the join
        if (own_failure != 1 || peer_failed != N - 1 || used_after_free != 0 || !comms.aborted() || first.rank() != culprit ||
            told != "injected on rank " + std::to_string(culprit)) {
            printf("round %d: own %d peers %d used-after-free %d first %d told [%s]\n", round, own_failure.load(), peer_failed.load(),
                   used_after_free.load(), first.rank(), told.c_str());
            ++bad;
        }
    }
    printf("%d rounds, %d bad\n", rounds, bad);
    printf("%d rounds with a blocking call\n", blocking_rounds);
    return bad ? 1 : 0;
}
