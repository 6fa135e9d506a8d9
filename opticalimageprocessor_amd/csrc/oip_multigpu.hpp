// oip_multigpu.hpp -- the two strip work-flows on the N GPUs of one node, in C++ over RCCL.
//
// `oip --gpus N ...` (default action, BASELINE config 4) and `oip prestitch --gpus N ...` (cross-CCD path,
// BASELINE config 5).  One process, one host thread and one oip_ctx per GPU, one RCCL communicator per GPU
// (ncclCommInitAll); librccl is loaded by the first --gpus run (dlopen, below): neither the CLI nor liboipgpu.so links it.  The strip is cut into
// scan-line blocks: rank r owns lines [r L/N, (r+1) L/N) of every raster and reads exactly those
// bytes of the input files.  Three exchange steps, none of them a reduction over pixels -- the same plan as
// opticalimageprocessor_amd/dist.py, whose gloo tests check it against the single-process result bit for bit;
// tests/test_cli_cpu.py compares the two plans through `oip plan`:
//   1. correlation windows: the reference correlates a fixed number of windows per strip (preproc.h:245-259,
//      stitcher.h:151-168; their geometry is oip_corrgeom.h's, which the single-GPU hosts and the C ABI's whole-strip
//      calls share); the (section, slice) units are placed by predicted cost (assign_groups_by_cost: a pair
//      moves only when bytes / link bandwidth beats computing it at home) and the lines a unit's rank lacks arrive as
//      compact windows: one grouped ncclSend / ncclRecv per pair on a communication stream, under the resident
//      pairs' kernels; a received pair is computed behind its own event;
//   2. ncclAllGather of the per-unit results, then the identical fixed-order host step on every rank
//      (filter + polynomial fit, or the CCD shift mean): bit-identical maps everywhere;
//   3. resampling halo (oip_align_mss_src_range / oip_remap_shift_src_range): whole lines, ncclSend / ncclRecv.
// Section seams come from GLOBAL line indices, so the blocks put together are the single-GPU product.
//
// The plans (placement, window pieces, halo lines, `oip plan`) are pure arithmetic: oip_nodeplan.hpp.  In here: the RCCL table,
// the stage clock, each rank's device memory, the Node (contexts, streams, communicators, rank threads, the three exchange
// steps, and exchange_and_correlate: steps 1 and 2 around the correlation, for both work-flows), then the two work-flows.
#pragma once

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <limits>
#include <thread>

#include <dlfcn.h>

#include "oip_host.hpp"
#include "oip_loopcomm.hpp"
#include "oip_nodeplan.hpp"
#include "oip_rankguard.hpp"

// RCCL is loaded when the first --gpus run asks for it, not with the executable: a single-GPU `oip` run then depends on
// libamdhip64 alone (what liboipgpu.so depends on), and a machine without RCCL can still run it.  It is not a start-up
// optimisation: an executable linked against the 570 MB librccl.so starts in 13.8 ms, this one in 12.5 ms
// (profiles/experiments/rccl_link_probe, `--version`, best of five each).  Types come from <rccl/rccl.h>; the entry points
// are resolved from librccl.so.1 on first use into RcclApi, through which the Node calls them (api.Send(...)).
//
// OIP_COMM=loopback (TEST ONLY) fills the same table from oip_loopcomm.hpp instead: the N ranks meet inside the process and all
// use one GPU (OIP_LOOPBACK_DEVICE, default 0), so every line of this host runs with N > 1 on a one-GPU machine -- real device
// buffers, streams and events, a device-to-device copy per matched send / receive.  librccl.so is not loaded in that mode.  It
// proves the host's ordering and addressing, not RCCL's behaviour or any link rate.
namespace OIPGPU {
// the loopback communicator under RCCL's signatures; ncclComm_t is an opaque pointer, a LoopComm stands behind it
struct LoopbackRccl {
    static LoopDeviceOps hip_ops()
    {
        LoopDeviceOps o;
        o.record = [](void *stream) -> void * {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            if (hipEventRecord(e, (hipStream_t)stream) != hipSuccess) { hipEventDestroy(e); return nullptr; }
            return e;
        };
        o.wait = [](void *stream, void *event) { return hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0) == hipSuccess; };
        o.copy = [](void *dst, const void *src, size_t bytes, void *stream) {
            return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess;
        };
        o.release = [](void *event) { hipEventDestroy((hipEvent_t)event); };
        return o;
    }
    static ncclResult_t rc(int e) { return e ? ncclInternalError : ncclSuccess; }
    static LoopComm *lc(ncclComm_t c) { return reinterpret_cast<LoopComm *>(c); }
    static size_t bytes_of(ncclDataType_t t)                                           // the host sends ncclUint8 and gathers ncclDouble
    {
        if (t == ncclUint8) return 1;
        if (t == ncclDouble) return 8;
        throw std::invalid_argument("loopback communicator: only ncclUint8 and ncclDouble are bound");
    }
    static ncclResult_t CommInitAll(ncclComm_t *comms, int n, const int *)             // (repeated device ids are what it is for)
    {
        const std::vector<LoopComm *> v = loop_init_all(n, hip_ops());
        for (int i = 0; i < n; ++i) comms[i] = reinterpret_cast<ncclComm_t>(v[(size_t)i]);
        return ncclSuccess;
    }
    static ncclResult_t CommDestroy(ncclComm_t c) { return rc(loop_destroy(lc(c))); }
    static ncclResult_t CommAbort(ncclComm_t c) { return rc(loop_abort(lc(c))); }     // wakes and fails; CommDestroy frees
    static ncclResult_t GroupStart() { return rc(loop_group_start()); }
    static ncclResult_t GroupEnd() { return rc(loop_group_end()); }
    static ncclResult_t Send(const void *buf, size_t count, ncclDataType_t t, int peer, ncclComm_t c, hipStream_t s)
    {
        return rc(loop_send(lc(c), buf, count * bytes_of(t), peer, s));
    }
    static ncclResult_t Recv(void *buf, size_t count, ncclDataType_t t, int peer, ncclComm_t c, hipStream_t s)
    {
        return rc(loop_recv(lc(c), buf, count * bytes_of(t), peer, s));
    }
    static ncclResult_t AllGather(const void *send, void *recv, size_t count, ncclDataType_t t, ncclComm_t c, hipStream_t s)
    {
        return rc(loop_allgather(lc(c), send, recv, count * bytes_of(t), s));
    }
    static const char *GetErrorString(ncclResult_t) { return loop_last_error(); }       // (of the calling thread's last call)
};

// the entry points the host calls, stated once: RcclApi's members, their loopback binding and their librccl binding follow from it
#define OIP_RCCL_CALLS(X) X(CommInitAll) X(CommDestroy) X(CommAbort) X(GroupStart) X(GroupEnd) X(Send) X(Recv) X(AllGather) X(GetErrorString)

struct RcclApi {
    bool loopback = false;
    int loopback_device = 0;
#define OIP_RCCL_MEMBER(name) decltype(&::nccl##name) name;
    OIP_RCCL_CALLS(OIP_RCCL_MEMBER)
#undef OIP_RCCL_MEMBER
    static RcclApi &get()
    {
        static RcclApi a;
        return a;
    }
private:
    RcclApi()
    {
        const char *mode = getenv("OIP_COMM");
        if (mode && !strcmp(mode, "loopback")) {
            loopback = true;
            if (const char *d = getenv("OIP_LOOPBACK_DEVICE")) loopback_device = atoi(d);
#define OIP_RCCL_LOOPBACK(name) name = &LoopbackRccl::name;
            OIP_RCCL_CALLS(OIP_RCCL_LOOPBACK)
#undef OIP_RCCL_LOOPBACK
            return;
        }
        if (mode && *mode && strcmp(mode, "rccl")) throw std::runtime_error(std::string("OIP_COMM: rccl or loopback expected, not ") + mode);
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) throw std::runtime_error(std::string("--gpus needs RCCL: ") + dlerror());
        auto sym = [&](const char *name) {
            void *p = dlsym(h, name);
            if (!p) throw std::runtime_error(std::string("librccl.so.1 lacks ") + name);
            return p;
        };
#define OIP_RCCL_SYMBOL(name) name = (decltype(name))sym("nccl" #name);
        OIP_RCCL_CALLS(OIP_RCCL_SYMBOL)
#undef OIP_RCCL_SYMBOL
    }
};

// ---- stage times of a rank's step -------------------------------------------------------------------
// The placement model (predicted_finish_us) has never met a multi-GPU node: every N-GPU run logs, per GPU, where its step's
// time went -- host time between points at which the rank's stream is drained anyway (RRC done, a correlation call returned,
// the all-gather or halo exchange synchronised, the product block downloaded) -- next to the model's prediction.
struct StageClock {
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    std::vector<std::pair<std::string, double>> ms;
    double since_rrc = 0.0, correlation_finish = 0.0;
    bool rrc_done = false;
    void tick(const char *name)
    {
        const auto now = std::chrono::steady_clock::now();
        const double d = std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
        for (auto &e : ms) if (e.first == name) { e.second += d; goto booked; }
        ms.push_back({name, d});
    booked:
        if (rrc_done) since_rrc += d;
        if (!strcmp(name, "rrc")) rrc_done = true;
        if (!strncmp(name, "correlate", 9)) correlation_finish = since_rrc;
    }
    std::string line() const
    {
        std::string s;
        char b[96];
        for (auto &e : ms) { snprintf(b, sizeof b, "%s%s %.2f", s.empty() ? "" : " | ", e.first.c_str(), e.second); s += b; }
        return s;
    }
};
inline void LogStageClocks(const std::vector<StageClock> &clk, const std::vector<long> &predicted_us)
{
    OLOG("Stage times per GPU in ms (host clock at points where the GPU's stream is drained; link figure assumed by the placement: %ld GB/s):", link_gbs());
    for (size_t r = 0; r < clk.size(); ++r) RLOG("  GPU %zu: %s", r, clk[r].line().c_str());
    std::string p, m;
    char b[48];
    for (size_t r = 0; r < clk.size(); ++r) {
        snprintf(b, sizeof b, "%s%ld", r ? ", " : "", r < predicted_us.size() ? predicted_us[r] : -1L); p += b;
        snprintf(b, sizeof b, "%s%.0f", r ? ", " : "", clk[r].correlation_finish * 1e3); m += b;
    }
    RLOG("  correlation stage finished (us after the RRC): predicted [%s], measured [%s]", p.c_str(), m.c_str());
}

// ---- a rank's device memory ---------------------------------------------------------------------------------------------
// alloc() hands out a pointer, release() frees one early (to cap HBM use), the destructor frees what is left.  The Node holds
// one per rank: run() empties it when the rank's step has returned; after a failure ~Node does, when every rank thread has
// joined -- not while the failed rank unwinds, where hipFree would wait for the device before run() has aborted the
// communicators that the device may be waiting on.
struct RankMem {
    oip_ctx *ctx = nullptr;
    std::vector<void *> held;
    RankMem() = default;
    RankMem(const RankMem &) = delete;
    RankMem &operator=(const RankMem &) = delete;
    ~RankMem() { release_all(); }
    int alloc(void **p, size_t bytes)
    {
        const int rc = oip_malloc(ctx, p, bytes);
        if (rc == OIP_OK) held.push_back(*p);
        return rc;
    }
    int release(void *p)                        // (null: nothing to do)
    {
        const auto it = std::find(held.begin(), held.end(), p);
        if (it == held.end()) return OIP_OK;
        held.erase(it);
        return oip_free(ctx, p);
    }
    void release_all() { while (!held.empty()) release(held.back()); }
};

// ---- the node: one context, stream and communicator per GPU, one host thread per GPU -------------------------------
class Node {
public:
    explicit Node(int n) : N(n), bar(n), ctx(n, nullptr), comms(n), first(n), mem(n), dev_of(n), window_stats(n)
    {
        loopback = api.loopback;
        int have = 0;
        if (hipGetDeviceCount(&have) != hipSuccess) have = 0;
        if (loopback) {
            if (api.loopback_device < 0 || api.loopback_device >= have)
                throw std::runtime_error("OIP_LOOPBACK_DEVICE " + std::to_string(api.loopback_device) + ": only " + std::to_string(have) + " GPUs visible");
        } else if (have < n)
            throw std::runtime_error("--gpus " + std::to_string(n) + ": only " + std::to_string(have) + " GPUs visible");
        for (int i = 0; i < n; ++i) {
            dev_of[i] = loopback ? api.loopback_device : i;
            if (oip_create(dev_of[i], &ctx[i]) != OIP_OK) throw std::runtime_error("no usable MI355X (gfx950) device " + std::to_string(dev_of[i]));
            mem[i].ctx = ctx[i];
        }
        if (api.CommInitAll(comms.comm.data(), n, dev_of.data()) != ncclSuccess) throw std::runtime_error("ncclCommInitAll failed");
        // a communication stream per GPU: the window exchange runs on it, beside the compute stream's kernels
        cstream.assign(n, nullptr);
        for (int i = 0; i < n; ++i) {
            if (hipSetDevice(dev_of[i]) != hipSuccess || hipStreamCreateWithFlags(&cstream[i], hipStreamNonBlocking) != hipSuccess)
                throw std::runtime_error("communication stream of GPU " + std::to_string(i));
        }
    }
    ~Node()
    {
        // (the rank threads have joined: run() returned or never started)  Rank buffers, streams, communicators, contexts:
        for (size_t i = 0; i < mem.size(); ++i) { hipSetDevice(dev_of[i]); mem[i].release_all(); }
        for (size_t i = 0; i < cstream.size(); ++i) if (cstream[i]) { hipSetDevice(dev_of[i]); hipStreamDestroy(cstream[i]); }
        // ncclCommAbort has already freed RCCL's communicators; the loopback's abort only wakes and fails, its destroy frees
        if (!comms.aborted() || loopback) for (auto c : comms.comm) if (c) api.CommDestroy(c);
        for (auto c : ctx) if (c) oip_destroy(c);
    }
    hipStream_t stream(int r) { return (hipStream_t)oip_get_stream(ctx[r]); }
    void check(int r, int rc)
    {
        if (rc == OIP_OK) return;
        const std::string m = oip_last_error(ctx[r]);
        if (rc == OIP_E_INVALID) throw std::invalid_argument(m);
        throw std::runtime_error(m);
    }
    // `count` elements of rank r's device memory; freed by release(), or with the rest when the rank's step is over (RankMem)
    template <typename T> T *alloc(int r, size_t count)
    {
        void *p = nullptr;
        check(r, mem[r].alloc(&p, count * sizeof(T)));
        return (T *)p;
    }
    int release(int r, void *p) { return mem[r].release(p); }
    // a rank's lines, read from a file at its block's offset.  A short read would leave uninitialised HBM under the
    // correlation: the block must arrive whole (as DevBuf::load_file checks)
    void read_block(int r, const std::string &file, size_t offset, size_t bytes, void *dst)
    {
        size_t got = 0;
        check(r, oip_read_file_to_device(ctx[r], file.c_str(), offset, bytes, dst, &got, nullptr));
        if (got != bytes)
            throw std::runtime_error("read file [" + file + "] failed: " + std::to_string(got) + " of " + std::to_string(bytes) +
                                     " bytes at offset " + std::to_string(offset));
    }
    // run fn(rank) on one thread per GPU; the exception of the rank that failed first is re-thrown on the caller
    template <typename F> void run(F fn)
    {
        std::vector<std::thread> th;
        for (int r = 0; r < N; ++r)
            th.emplace_back([&, r] {
                try { hipSetDevice(dev_of[r]); fn(r); mem[r].release_all(); }
                catch (...) {
                    // A rank that gives up after a pre-exchange barrier leaves its peers inside a grouped send/recv, blocked in
                    // oip_sync on a kernel that waits for this rank for ever: setting a flag does not unblock a device-side wait.
                    // Aborting every communicator makes those kernels exit, the peers' streams drain, their oip_sync returns
                    // and they leave through sync_point(); the process then exits non-zero with this rank's message.
                    // The failure is noted BEFORE anything that makes the peers fail: what they raise afterwards (PeerFailed, or
                    // the error of a call that the abort released, see nccl_ok) is a consequence, whatever their rank index.
                    first.note(r, std::current_exception()); bar.abort(); abort_comms();
                }
            });
        for (auto &t : th) t.join();
        first.rethrow();                    // the rank that failed first tells why
    }
    bool failed() const { return first.any(); }
    // every rank thread calls this at the same point; a failure on any rank is raised on all (no rank is left waiting
    // in a collective for a peer that has given up)
    void sync_point()
    {
        if (!bar.wait() || failed()) throw PeerFailed();
    }
    // aborts every communicator once, without waiting for the calls in flight on the peers' threads (CommGuard): a peer may
    // be blocked in one until this rank arrives, and the abort is what releases it.  From the first abort on with_comm()
    // throws PeerFailed.  (ncclCommAbort also frees: RCCL allows it beside a call in flight on that communicator, but a call
    // that passed with_comm()'s check and has not entered RCCL yet would meet a freed communicator -- a window of a few
    // instructions that only a run on real RCCL with N > 1 could show; the loopback's abort frees nothing.)
    void abort_comms()
    {
        comms.abort_all([this](ncclComm_t c) { if (c) api.CommAbort(c); });
    }
    // every use of a communicator -- one call or a whole ncclGroupStart .. ncclGroupEnd sequence -- goes through here
    template <typename F> void with_comm(int r, F f)
    {
        if (failed()) throw PeerFailed();
        comms.use(r, f);
    }
    // an RCCL call that fails is this rank's failure: raised at once (run() then aborts the communicators), never carried
    // into a stream synchronisation that a peer may not be able to complete.  Once the node has failed it is a consequence
    // of the abort instead: PeerFailed, so that run() reports the culprit and not this call
    void nccl_ok(ncclResult_t rc, const char *what)
    {
        if (rc == ncclSuccess) return;
        if (failed()) throw PeerFailed();
        throw std::runtime_error(std::string(what) + " failed: " + api.GetErrorString(rc));
    }

    // exchange step 1, overlapped with the correlation: every group of units that is not entirely on its rank is packed and
    // posted as ONE grouped send/recv on the rank's communication stream, in the global order every rank iterates; an event
    // per group lets the compute stream wait for that group's bytes only.  exchange_and_correlate (below) computes the resident
    // groups first, then each received group behind its event, and finally calls finish_pieces (drains the stream, frees the
    // packing buffers, meets the other ranks).
    struct PendingExchange {
        std::vector<hipEvent_t> events;         // one per exchange group
        std::vector<void *> temps;
    };
    // src_of(piece, plane) -> (pointer, pitch in pixels) of the piece's lines on this rank; dst_of(piece, plane) -> their place in
    // the window buffer of the piece's unit on this rank; planes_of(kind): the planes a piece of that kind has
    template <typename PlanesOf, typename SrcOf, typename DstOf>
    PendingExchange post_pieces(int r, const std::vector<ExchangeGroup> &groups, PlanesOf planes_of, SrcOf src_of, DstOf dst_of)
    {
        PendingExchange pe;
        hipStream_t st = stream(r), cs = cstream[r];
        // the communication stream starts behind what the compute stream has produced so far (the corrected lines)
        hipEvent_t ready;
        if (hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess || hipEventRecord(ready, st) != hipSuccess ||
            hipStreamWaitEvent(cs, ready, 0) != hipSuccess) throw std::runtime_error("communication stream ordering failed");
        hipEventDestroy(ready);
        sync_point();
        for (const ExchangeGroup &g : groups) {
            struct Xfer { void *buf; size_t bytes; int peer; };
            std::vector<Xfer> sends, recvs;
            for (const Piece &p : g.pieces) {
                for (int b = 0; b < planes_of(p.kind); ++b) {
                    const size_t bytes = (size_t)p.rows * p.cols * 2;
                    if (p.src == r && p.dst == r) {
                        auto s = src_of(p, b);
                        if (hipMemcpy2DAsync(dst_of(p, b), (size_t)p.cols * 2, s.first, s.second * 2, (size_t)p.cols * 2, p.rows,
                                             hipMemcpyDeviceToDevice, cs) != hipSuccess) throw std::runtime_error("window copy failed");
                    } else if (p.src == r) {
                        void *t = alloc<uint8_t>(r, bytes);
                        pe.temps.push_back(t);
                        auto s = src_of(p, b);
                        if (hipMemcpy2DAsync(t, (size_t)p.cols * 2, s.first, s.second * 2, (size_t)p.cols * 2, p.rows,
                                             hipMemcpyDeviceToDevice, cs) != hipSuccess) throw std::runtime_error("window pack failed");
                        sends.push_back({t, bytes, p.dst});
                    } else if (p.dst == r) {
                        recvs.push_back({dst_of(p, b), bytes, p.src});
                    }
                }
            }
            if (!sends.empty() || !recvs.empty())
                with_comm(r, [&](ncclComm_t c) {
                    fault_point(r, "exchange");
                    nccl_ok(api.GroupStart(), "ncclGroupStart");
                    for (auto &x : sends) nccl_ok(api.Send(x.buf, x.bytes, ncclUint8, x.peer, c, cs), "ncclSend (window piece)");
                    for (auto &x : recvs) nccl_ok(api.Recv(x.buf, x.bytes, ncclUint8, x.peer, c, cs), "ncclRecv (window piece)");
                    nccl_ok(api.GroupEnd(), "ncclGroupEnd");
                });
            hipEvent_t ev;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, cs) != hipSuccess)
                throw std::runtime_error("exchange event failed");
            pe.events.push_back(ev);
        }
        return pe;
    }
    void finish_pieces(int r, PendingExchange *pe)
    {
        if (hipStreamSynchronize(cstream[r]) != hipSuccess) throw std::runtime_error("window exchange failed");
        for (hipEvent_t ev : pe->events) hipEventDestroy(ev);
        for (void *t : pe->temps) release(r, t);
        if (loopback) window_stats[r] = loop_stats(LoopbackRccl::lc(comms.comm[r]));
        sync_point();
    }

    // Exchange 1, the correlation and exchange 2 of both work-flows.  The plan's groups (pairs (2k, 2k+1) of inter-band units,
    // single CCD sections) are computed whole, as the single-GPU order computes them: this rank's entirely local groups while the
    // exchange runs on the communication stream, then every group it receives behind its own event, in posting order.  With
    // an odd slice count a pair spans two sections and one unit can be local while its partner is not -- computing the local
    // one alone would shift every later pairing on this rank, and a unit's last digits depend on its partner: such
    // a pair waits for its exchange group.  (The plan places groups: a group is this rank's or not as a whole.)
    // after_post() books the stage clock behind the post, where the work-flows differ; correlate(units, win) computes units into
    // the table; win[u][kind] is the unit's received window, planes one behind the other, or null where it reads the rank's own
    // lines.  Returns the window buffers: they are the rank's (RankMem); a caller that goes on to need the HBM releases them.
    using Windows = std::vector<std::array<uint16_t *, 2>>;
    template <typename Plan, typename SrcOf, typename AfterPost, typename Correlate>
    Windows exchange_and_correlate(int r, const Plan &plan, StageClock &clk, std::vector<double> *table, int stride, SrcOf src_of,
                                   AfterPost after_post, Correlate correlate)
    {
        const std::vector<int> mine = plan.units_of(r);
        const std::vector<Window> shape = plan.unit_windows(0);            // (rows, columns and planes are the same for every unit)
        Windows win((size_t)plan.n_units, {nullptr, nullptr});
        for (int u : mine)
            if (!plan.unit_is_local(u))
                for (int k = 0; k < 2; ++k) win[u][k] = alloc<uint16_t>(r, (size_t)shape[k].rows * shape[k].cols * shape[k].planes);
        const std::vector<ExchangeGroup> groups = plan.exchange_groups();
        PendingExchange pending = post_pieces(
            r, groups, [&](int kind) { return shape[kind].planes; }, src_of,
            [&](const Piece &p, int b) -> void * { return win[p.unit][p.kind] + ((size_t)b * shape[p.kind].rows + p.dst_row) * shape[p.kind].cols; });
        after_post();
        std::vector<int> resident;
        for (int u : mine) if (plan.group_is_local(plan.group_of(u))) resident.push_back(u);
        if (!resident.empty()) correlate(resident, win);
        clk.tick("correlate_resident");
        for (size_t i = 0; i < groups.size(); ++i) {
            if (plan.assign[groups[i].units[0]] != r) continue;
            // the compute stream waits (on the device) for the group's bytes; the host waits too (the correlation call that follows
            // could not start earlier anyway): the wait is then booked apart from the group's correlation (StageClock)
            if (hipEventSynchronize(pending.events[i]) != hipSuccess || hipStreamWaitEvent(stream(r), pending.events[i], 0) != hipSuccess)
                throw std::runtime_error("exchange wait failed");
            clk.tick("exchange_wait");
            correlate(groups[i].units, win);
            clk.tick("correlate_received");
        }
        finish_pieces(r, &pending);
        clk.tick("exchange_drain");
        allgather_table(r, table, stride);
        clk.tick("allgather");
        return win;
    }
    // OIP_COMM=loopback: what every rank sent and received, for the test that compares it with the plan's sums
    void log_loopback_accounting()
    {
        if (!loopback) return;
        for (int r = 0; r < N; ++r) {
            const LoopStats s = loop_stats(LoopbackRccl::lc(comms.comm[r])), &w = window_stats[r];
            RLOG("loopback: GPU %d sent %ld bytes in %ld sends, received %ld bytes in %ld receives", r, s.send_bytes, s.sends, s.recv_bytes, s.recvs);
            RLOG("loopback: GPU %d window exchange alone: sent %ld bytes in %ld sends, received %ld bytes in %ld receives; %ld all-gathers of %ld bytes",
                 r, w.send_bytes, w.sends, w.recv_bytes, w.recvs, s.gathers, s.gather_bytes);
        }
    }

    // exchange step 3: whole lines into the halo rows of a raster.  ptr_of(global line, plane) -> device pointer on
    // this rank; bytes_per_line per plane
    template <typename PtrOf>
    void exchange_lines(int r, const std::vector<LineTransfer> &tr, int planes, size_t bytes_per_line, PtrOf ptr_of)
    {
        hipStream_t st = stream(r);
        sync_point();
        bool any = false;
        for (const LineTransfer &t : tr) any = any || t.src == r || t.dst == r;
        if (any)
            with_comm(r, [&](ncclComm_t c) {
                fault_point(r, "halo");
                nccl_ok(api.GroupStart(), "ncclGroupStart");
                for (const LineTransfer &t : tr)
                    for (int b = 0; b < planes; ++b) {
                        if (t.src == r) nccl_ok(api.Send(ptr_of(t.row0, b), (size_t)t.rows * bytes_per_line, ncclUint8, t.dst, c, st), "ncclSend (halo lines)");
                        if (t.dst == r) nccl_ok(api.Recv(ptr_of(t.row0, b), (size_t)t.rows * bytes_per_line, ncclUint8, t.src, c, st), "ncclRecv (halo lines)");
                    }
                nccl_ok(api.GroupEnd(), "ncclGroupEnd");
            });
        check(r, oip_sync(ctx[r]));
        sync_point();
    }

    // exchange step 2: every rank contributes a table with NaN for what it did not compute; all ranks end with the merged
    // table (rank order, first non-NaN wins -- each entry is computed by exactly one rank)
    void allgather_table(int r, std::vector<double> *table, int stride)
    {
        const size_t n = table->size();
        double *d_send = alloc<double>(r, n), *d_recv = alloc<double>(r, n * N);
        check(r, oip_memcpy_h2d(ctx[r], d_send, table->data(), n * sizeof(double)));
        check(r, oip_sync(ctx[r]));
        sync_point();
        with_comm(r, [&](ncclComm_t c) {
            fault_point(r, "allgather");
            nccl_ok(api.AllGather(d_send, d_recv, n, ncclDouble, c, stream(r)), "ncclAllGather");
        });
        std::vector<double> all(n * N);
        check(r, oip_memcpy_d2h(ctx[r], all.data(), d_recv, n * N * sizeof(double)));
        check(r, oip_sync(ctx[r]));
        for (size_t i = 0; i < n; i += stride)
            for (int q = 0; q < N; ++q)
                if (all[q * n + i] == all[q * n + i]) { for (int k = 0; k < stride; ++k) (*table)[i + k] = all[q * n + i + k]; break; }
        release(r, d_send);
        release(r, d_recv);
        sync_point();
    }

    const int N;
    HostBarrier bar;
    // OIP_FAULT_INJECT="<rank>:<point>" (point: exchange, halo, allgather) makes that rank throw at that point -- behind the
    // barrier that precedes the exchange, its peers already posting: what the failure path has to survive (test_gpu_cli.py)
    static void fault_point(int r, const char *point)
    {
        const char *e = getenv("OIP_FAULT_INJECT");
        if (!e) return;
        char want[32] = "";
        int rank = -1;
        if (sscanf(e, "%d:%31s", &rank, want) == 2 && rank == r && !strcmp(want, point))
            throw std::runtime_error(std::string("injected failure on GPU ") + std::to_string(r) + " at " + point);
    }

    std::vector<oip_ctx *> ctx;
    CommGuard<ncclComm_t> comms;
    std::vector<hipStream_t> cstream;
    FirstFailure first;
    std::vector<RankMem> mem;
    const RcclApi &api = RcclApi::get();
    bool loopback = false;
    std::vector<int> dev_of;                    // rank -> HIP device: the identity, or OIP_LOOPBACK_DEVICE for every rank
    std::vector<LoopStats> window_stats;        // the loopback's accounting when the window exchange had drained
};

struct MultiGpuDefaultOptions : PreProcessor::DefaultActionOptions {      // (no --write-rrcpan with --gpus)
    int width = OIP_PIXELS_PER_LINE, gpus = 1, fitMode = OIP_FIT_REFERENCE;
};

// main.cpp:288-317 on N GPUs: <stem>.ALIGNED.TIFF is the single-GPU product
inline void RunDefaultActionMultiGpu(const std::string &panFile, const std::string &mssFile, const std::string &rrcPan,
                                     const std::string rrcMss[MSS_BANDS], const MultiGpuDefaultOptions &o)
{
    const int W = o.width, Wb = W / MSS_BANDS, N = o.gpus;
    const size_t lineBytes = (size_t)W * BYTES_PER_PIXEL;
    const size_t sizePAN = IMO::FileSize(panFile), sizeMSS = IMO::FileSize(mssFile);
    PreProcessor::CheckStripSizes(sizePAN, sizeMSS, lineBytes);
    const long Lp = (long)(sizePAN / lineBytes);
    StripPlanC plan(W, Lp, N, o.slices, o.sections, OIP_CORRELATION_LINES, o.linesSection, o.lineOffset, o.overlapLines, o.keepLeading);
    OLOG("Strip of %ld PAN lines on %d GPUs: %ld lines per GPU, %d correlation units dealt %s.", Lp, N, plan.pb, plan.n_units,
         plan.correlation_pieces().empty() ? "without moving a line" : "with window exchange");
    std::vector<double> kbPan, kbMss;
    if (o.doRRC4PAN) kbPan = IMO::LoadLut(rrcPan, W);
    if (o.doRRC4MSS) kbMss = IMO::LoadMssLuts(rrcMss, W);
    Node node(N);
    std::vector<std::vector<uint16_t>> blocks(N);             // aligned rows of each rank, on the host
    std::vector<std::pair<long, long>> out_rows(N);
    double cxAll[MSS_BANDS][2] = {}, cyAll[MSS_BANDS][3] = {};
    std::vector<StageClock> clocks(N);
    node.run([&](int r) {
        StageClock &clk = clocks[r];
        oip_ctx *c = node.ctx[r];
        auto ck = [&](int rc) { node.check(r, rc); };
        // the rank's own lines, read from the files at the block's offset
        const long b0 = r * plan.mb, b1 = (r + 1) * plan.mb;
        const long head = std::min<long>(plan.halo_cap, b0), tail = std::min<long>(plan.halo_cap, plan.Lm - b1);
        const long m_first = b0 - head, m_cap = head + plan.mb + tail;
        const size_t plane_stride = (size_t)m_cap * Wb;
        uint16_t *pan = node.alloc<uint16_t>(r, (size_t)plan.pb * W), *bil = node.alloc<uint16_t>(r, (size_t)plan.mb * W);
        uint16_t *planes = node.alloc<uint16_t>(r, plane_stride * MSS_BANDS);
        ck(oip_memset(c, planes, 0, plane_stride * MSS_BANDS * 2));
        node.read_block(r, panFile, (size_t)r * plan.pb * lineBytes, (size_t)plan.pb * lineBytes, pan);
        node.read_block(r, mssFile, (size_t)r * plan.mb * lineBytes, (size_t)plan.mb * lineBytes, bil);
        ck(oip_sync(c));
        clk.tick("read");
        double *d_kb = node.alloc<double>(r, (size_t)W * 2);
        if (o.doRRC4PAN) {
            ck(oip_memcpy_h2d(c, d_kb, kbPan.data(), (size_t)W * 16));
            ck(oip_rrc_u16(c, pan, pan, W, plan.pb, d_kb));
            ck(oip_sync(c));
        }
        if (o.doRRC4MSS) ck(oip_memcpy_h2d(c, d_kb, kbMss.data(), (size_t)W * 16));
        uint16_t *own = planes + (size_t)head * Wb;
        ck(oip_mss_split_rrc_u16(c, bil, own, plane_stride, W, plan.mb, o.doRRC4MSS ? d_kb : nullptr));
        ck(oip_sync(c));
        clk.tick("rrc");
        ck(node.release(r, bil));
        // exchange 1 (compact windows of the units this rank computes but does not hold entirely), the correlation under it, and
        // exchange 2: the table [unit][band][dx, dy, rs]
        std::vector<double> table((size_t)plan.n_units * 12, std::numeric_limits<double>::quiet_NaN());
        node.exchange_and_correlate(
            r, plan, clk, &table, 12,
            [&](const Piece &p, int b) -> std::pair<const void *, size_t> {
                if (p.kind == 0) return {pan + (size_t)(p.row0 - r * plan.pb) * W + p.col0, (size_t)W};
                return {planes + (size_t)b * plane_stride + (size_t)(p.row0 - m_first) * Wb + p.col0, (size_t)Wb};
            },
            [&] { clk.tick("exchange_post"); },
            [&](const std::vector<int> &units, const Node::Windows &win) {
                std::vector<const uint16_t *> up, ub;
                std::vector<size_t> pp, pbm;
                for (int u : units) {
                    const long p0 = plan.pan_start(u / plan.slices), m0 = plan.mss_start(u / plan.slices);
                    const int i = u % plan.slices;
                    if (win[u][0]) {
                        up.push_back(win[u][0]); pp.push_back(plan.base_cols);
                        for (int b = 0; b < MSS_BANDS; ++b) ub.push_back(win[u][1] + (size_t)b * plan.band_rows * plan.band_cols);
                        pbm.push_back(plan.band_cols);
                    } else {
                        up.push_back(pan + (size_t)(p0 - r * plan.pb) * W + (size_t)i * plan.base_cols); pp.push_back(W);
                        for (int b = 0; b < MSS_BANDS; ++b) ub.push_back(planes + (size_t)b * plane_stride + (size_t)(m0 - m_first) * Wb + (size_t)i * plan.band_cols);
                        pbm.push_back(Wb);
                    }
                }
                std::vector<double> res(12 * units.size() + 12);
                ck(oip_interband_correlate_units(c, up.data(), pp.data(), ub.data(), pbm.data(), (int)units.size(), plan.base_rows, plan.base_cols, res.data()));
                for (size_t j = 0; j < units.size(); ++j) memcpy(&table[(size_t)units[j] * 12], &res[12 * j], sizeof(double) * 12);
            });
        std::vector<double> shifts((size_t)MSS_BANDS * plan.n_units * 4);
        ShiftTableInit(plan, shifts.data());
        for (int u = 0; u < plan.n_units; ++u) ShiftTablePut(plan, shifts.data(), u, &table[(size_t)u * 12]);
        double cx[MSS_BANDS][2], cy[MSS_BANDS][3];
        char err[512];
        if (oip_filter_and_fit_mode(shifts.data(), plan.n_units, o.threshold, OIP_IBCV_MIN_COUNT, o.fitMode, &cx[0][0], &cy[0][0], err, sizeof err) != OIP_OK)
            throw std::runtime_error(err);
        if (r == 0) { memcpy(cxAll, cx, sizeof cx); memcpy(cyAll, cy, sizeof cy); }
        // exchange 3: align halo
        std::vector<std::pair<long, long>> need;
        auto tr = plan.align_transfers(&cy[0][0], &need);
        for (const LineTransfer &t : tr)
            if (t.dst == r && (t.row0 < m_first || t.row0 + t.rows > m_first + m_cap)) throw std::runtime_error("MSS halo exceeds buffer capacity");
        node.exchange_lines(r, tr, MSS_BANDS, (size_t)Wb * 2, [&](long line, int b) -> void * {
            return planes + (size_t)b * plane_stride + (size_t)(line - m_first) * Wb;
        });
        clk.tick("fit+halo");
        long v0 = b0, v1 = b1;
        for (const LineTransfer &t : tr) if (t.dst == r) { v0 = std::min(v0, t.row0); v1 = std::max(v1, t.row0 + t.rows); }
        long o0, o1;
        plan.align_out_rows(r, &o0, &o1);
        out_rows[r] = {o0, o1};
        if (o1 > o0) {
            const size_t n = (size_t)(o1 - o0) * Wb * MSS_BANDS;
            uint16_t *out = node.alloc<uint16_t>(r, n);
            ck(oip_align_mss_bicubic_u16x4(c, planes + (size_t)(v0 - m_first) * Wb, plane_stride, v0, v1 - v0, out, o0, o1 - o0, Wb, plan.Lm,
                                           &cx[0][0], &cy[0][0], o.linesSection, o.lineOffset, o.overlapLines, o.keepLeading ? 1 : 0,
                                           OIP_IBPA_MIN_PROCESSLINES, nullptr));
            blocks[r].resize(n);
            ck(oip_download_staged(c, blocks[r].data(), out, n * 2));
            ck(node.release(r, out));
        }
        clk.tick("align+download");
    });
    LogStageClocks(clocks, plan.predicted_finish_us);
    node.log_loopback_accounting();
    LogShiftCoeffs(cxAll, cyAll);
    // preproc.h:167-185: one ALIGNED.TIFF, the blocks in rank order
    auto save = IMO::BuildOutputFilePath(mssFile, ".ALIGNED", ".TIFF");
    OLOG("Outputing aligned TIFF image (%d x %ld x 4) to [%s] ...", Wb, plan.out_rows, save.c_str());
    TiffWriterU16 tw(save, Wb, plan.out_rows, MSS_BANDS, true, tiff_compression(TIFF_LZW));
    for (int r = 0; r < N; ++r)
        if (out_rows[r].second > out_rows[r].first) tw.write_rows(blocks[r].data(), out_rows[r].second - out_rows[r].first);
    tw.close();
    OLOG("Output done.");
}

struct MultiGpuPrestitchOptions {
    int width = OIP_PIXELS_PER_LINE, gpus = 1, sections = OIP_STT_DEF_SECTIONS, sectionLines = OIP_STT_DEF_SECLINES,
        overlapCols = OIP_STT_DEF_OVERLAPPX, edgeCols = 0;
    double threshold = OIP_STT_DEF_PHCTHRHLD, maxDeltaY = 0.0;
    bool doRRC = true, onlyCalc = false, fp16acc = false;
};

// main.cpp:270-286 on N GPUs: .RRC.RAW x 2 and .RRC.PRESTT.RAW are the single-GPU products
inline void RunPrestitchMultiGpu(const std::string &pan1, const std::string &pan2, const std::string &rrc1, const std::string &rrc2,
                                 const MultiGpuPrestitchOptions &o)
{
    const int W = o.width, N = o.gpus;
    const size_t lineBytes = (size_t)W * BYTES_PER_PIXEL;
    const size_t s1 = IMO::FileSize(pan1), s2 = IMO::FileSize(pan2);
    if (s1 != s2) throw std::invalid_argument("PAN1 size doesn't match PAN2 size");
    const long L = (long)(s1 / lineBytes);
    CcdPlanC plan(W, L, N, o.sections, o.sectionLines, o.overlapCols, o.edgeCols);
    OLOG("Strips of %ld lines on %d GPUs: %ld lines per GPU, %d correlation sections dealt %s.", L, N, plan.pb, plan.n_units,
         plan.correlation_pieces().empty() ? "without moving a line" : "with window exchange");
    if (!o.onlyCalc && L <= OIP_REMAP_ROW_GUARD) throw std::invalid_argument("too few data rows, please use cv::remap()");   // imageop.h:242-244
    std::vector<double> kb1, kb2;
    if (o.doRRC && !o.onlyCalc) {
        kb1 = IMO::LoadLut(rrc1, W);
        kb2 = IMO::LoadLut(rrc2, W);
    }
    const std::string f1 = o.doRRC ? IMO::BuildOutputFilePath(pan1, ".RRC") : pan1, f2 = o.doRRC ? IMO::BuildOutputFilePath(pan2, ".RRC") : pan2;
    const std::string fp = IMO::BuildOutputFilePath(f2, ".PRESTT");
    Node node(N);
    double dxAll = 0, dyAll = 0;
    std::vector<StageClock> clocks(N);
    node.run([&](int r) {
        StageClock &clk = clocks[r];
        oip_ctx *c = node.ctx[r];
        auto ck = [&](int rc) { node.check(r, rc); };
        const long b0 = r * plan.pb;
        const size_t blockBytes = (size_t)plan.pb * lineBytes;
        uint16_t *p1 = node.alloc<uint16_t>(r, (size_t)plan.pb * W), *p2 = node.alloc<uint16_t>(r, (size_t)plan.pb * W);
        node.read_block(r, pan1, (size_t)b0 * lineBytes, blockBytes, p1);
        node.read_block(r, pan2, (size_t)b0 * lineBytes, blockBytes, p2);
        ck(oip_sync(c));
        // exchange 1 + correlation on the RAW lines (App. B-1), and exchange 2: the table [section][dx, dy, response]
        std::vector<double> table((size_t)plan.sections * 3, std::numeric_limits<double>::quiet_NaN());
        const Node::Windows windows = node.exchange_and_correlate(
            r, plan, clk, &table, 3,
            [&](const Piece &p, int) -> std::pair<const void *, size_t> {
                return {(p.kind == 0 ? p1 : p2) + (size_t)(p.row0 - b0) * W + p.col0, (size_t)W};
            },
            [&] {
                ck(oip_sync(c));
                clk.tick("read");
                clk.tick("rrc");                          // CalcSttParameters works on the RAW lines: the model's time 0 is here
            },
            [&](const std::vector<int> &units, const Node::Windows &win) {
                std::vector<const uint16_t *> pa, pbv;
                std::vector<size_t> qa, qb;
                for (int u : units) {
                    if (win[u][0]) { pa.push_back(win[u][0]); pbv.push_back(win[u][1]); qa.push_back(plan.cols); qb.push_back(plan.cols); }
                    else {
                        const long a = plan.section_start(u);
                        pa.push_back(p1 + (size_t)(a - b0) * W + plan.col1); pbv.push_back(p2 + (size_t)(a - b0) * W + plan.col2);
                        qa.push_back(W); qb.push_back(W);
                    }
                }
                std::vector<double> res(3 * units.size() + 3);
                ck(oip_stt_correlate_windows(c, pa.data(), qa.data(), pbv.data(), qb.data(), (int)units.size(), plan.rows, plan.cols, res.data()));
                for (size_t j = 0; j < units.size(); ++j) memcpy(&table[(size_t)units[j] * 3], &res[3 * j], sizeof(double) * 3);
            });
        double dx, dy, resp;
        int valid = 0;
        if (oip_stt_mean(table.data(), plan.sections, o.threshold, o.maxDeltaY, &dx, &dy, &resp, &valid) != OIP_OK)      // stitcher.h:181-198
            throw std::runtime_error("No valid delta value found for stitching parameter calculating");
        if (r == 0) {
            dxAll = dx; dyAll = dy;
            RLOG("| offset |  delta x |  delta y | response | r |");
            for (int i = 0; i < plan.sections; ++i)
                RLOG("|%7ld |%10.4f|%10.4f|%10.4f|%s|", plan.section_start(i), table[3 * i], table[3 * i + 1], table[3 * i + 2],
                     (table[3 * i + 2] >= o.threshold && (o.maxDeltaY <= 0.0 || std::abs(table[3 * i + 1]) <= o.maxDeltaY)) ? " Y " : " N ");
            OLOG("Total %d valid delta value pairs found, everage value:", valid);
            OLOG("    dx: %.5f, dy: %.5f, r: %.5f", dx, dy, resp);
        }
        for (const auto &w : windows) for (uint16_t *p : w) node.release(r, p);         // the remap needs the HBM
        if (o.onlyCalc) return;
        // DoRRC of the rank's lines; CCD 2 lands in a buffer with room for the remap halo
        std::vector<std::pair<long, long>> need;
        auto tr = plan.remap_transfers(dy, &need);
        const long f = std::min(need[r].first, b0), l = std::max(need[r].second, b0 + plan.pb);
        uint16_t *r2 = node.alloc<uint16_t>(r, (size_t)(l - f) * W);
        ck(oip_memset(c, r2, 0, (size_t)(l - f) * lineBytes));
        uint16_t *own2 = r2 + (size_t)(b0 - f) * W;
        if (o.doRRC) {
            double *d_kb = node.alloc<double>(r, (size_t)W * 2);
            ck(oip_memcpy_h2d(c, d_kb, kb1.data(), (size_t)W * 16));
            ck(oip_rrc_u16(c, p1, p1, W, plan.pb, d_kb));
            ck(oip_sync(c));
            ck(oip_memcpy_h2d(c, d_kb, kb2.data(), (size_t)W * 16));
            ck(oip_rrc_u16(c, p2, own2, W, plan.pb, d_kb));
            ck(oip_sync(c));
            node.release(r, d_kb);
        } else {
            if (hipMemcpyAsync(own2, p2, blockBytes, hipMemcpyDeviceToDevice, node.stream(r)) != hipSuccess) throw std::runtime_error("copy failed");
            ck(oip_sync(c));
        }
        node.release(r, p2);
        clk.tick("rrc_x2");
        node.exchange_lines(r, tr, 1, lineBytes, [&](long line, int) -> void * { return r2 + (size_t)(line - f) * W; });
        clk.tick("halo");
        uint16_t *dst = node.alloc<uint16_t>(r, (size_t)plan.pb * W);
        auto fn = o.fp16acc ? oip_remap_shift_bicubic_u16_f16acc : oip_remap_shift_bicubic_u16;
        ck(fn(c, r2, f, l - f, dst, b0, plan.pb, W, L, dx, dy, OIP_REMAP_SECTION_ROWS, OIP_REMAP_ROW_GUARD));
        ck(oip_sync(c));
        clk.tick("remap");
        // products: the ranks append their blocks to the files in rank order (every rank passes N turns)
        for (int t = 0; t < N; ++t) {
            if (t == r) {
                if (o.doRRC) {
                    ck(oip_write_device_to_file(c, p1, blockBytes, f1.c_str(), r > 0));
                    ck(oip_write_device_to_file(c, own2, blockBytes, f2.c_str(), r > 0));
                }
                ck(oip_write_device_to_file(c, dst, blockBytes, fp.c_str(), r > 0));
            }
            node.sync_point();
        }
        clk.tick("write");
    });
    LogStageClocks(clocks, plan.predicted_finish_us);
    node.log_loopback_accounting();
    if (!o.onlyCalc) OLOG("Pre-stitched PAN2 written to file '%s' (dx %.5f, dy %.5f).", fp.c_str(), dxAll, dyAll);
}

}  // namespace OIPGPU
