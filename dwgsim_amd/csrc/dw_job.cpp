// dw_job.cpp -- the job level of the C-ABI (include/dwgsim_hip.h, dwgsim_hip_job_*): the whole of dwgsim_core() (src/dwgsim.c:419-1121) on any
// number of GPUs, behind five calls.  It is written on top of the context-level entry points of the same header (one context per device) and
// owns what a caller of those would otherwise have to choreograph:
//   * the scheduling arithmetic of the contig loop (dwgsim.c:519-625): pairs per contig, skip rules, region lengths, -N remainders;
//   * GROUPS: consecutive contigs up to a size are resident, walked and simulated together (a scaffold-level assembly costs one walk chain
//     and a few launches per group, not per contig); their sequence is staged once in page-locked memory and uploaded asynchronously;
//   * the pipeline of every device: upload + walk of group k+1 on the walk stream while the batches of group k run; two batches in flight;
//     finished text (or the gzip members made on the GPU) copied into page-locked buffers behind the kernels;
//   * SHARDING: the pairs of a group, in file order, are cut into batches of read-index ranges; batch b belongs to device b mod n.  Every
//     device walks every group itself (deterministic, cheap: no broadcast).  What crosses devices is two integers per batch -- the random-read
//     count in front of it (rand_ii, dwgsim.c:1042,1096: every device counts the random reads of its batches with k_place before it simulates,
//     one host-side prefix sum per group) and the abort rule's summary (dwgsim.c:635, :833-843; joined in order at the end of the group).
//     No collective, no RCCL, no device-to-device traffic;
//   * ORDER: one delivery thread per output stream hands the batches to the caller's sink in file order.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <stdarg.h>
#include <time.h>
#include <limits.h>
#include <algorithm>
#include <string>
#include <vector>
#include <deque>
#include <array>
#include <memory>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <atomic>
#include <sched.h>
#include "../../include/dwgsim_hip.h"

namespace {

// A device's worker thread -- it allocates the device's page-locked output buffers and waits for its copies -- runs on the cores of the NUMA node the
// GPU hangs off (dwgsim_hip_device_numa_node: /sys/bus/pci/devices/<bus id>/numa_node), so that on a two-socket node no device copies its members
// across the socket link.  Quietly does nothing where the node is unknown (-1: single-socket boxes, containers without sysfs), where the node's
// cores are not among the ones the process may use, or with DWGSIM_HIP_NO_PIN set.
void pin_thread_to_device_node(int device)
{
    if (getenv("DWGSIM_HIP_NO_PIN")) return;
    const int node = dwgsim_hip_device_numa_node(device);
    if (node < 0) return;
    char path[128]; snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = fopen(path, "r");
    if (!f) return;
    char list[4096]; const bool got = fgets(list, sizeof list, f) != nullptr; fclose(f);
    if (!got) return;
    cpu_set_t allowed, want; CPU_ZERO(&allowed); CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return;
    int n_want = 0;
    for (const char *q = list; *q && *q != '\n';) {      // "0-31,64-95"
        char *e; long a = strtol(q, &e, 10), b = a;
        if (e == q) break;
        if (*e == '-') { q = e + 1; b = strtol(q, &e, 10); }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) if (CPU_ISSET((int)c, &allowed)) { CPU_SET((int)c, &want); ++n_want; }
        q = *e == ',' ? e + 1 : e;
    }
    if (n_want > 0) (void)sched_setaffinity(0, sizeof want, &want);
}

// ---- owners ----
// Page-locked host memory through the public ABI alone (dwgsim_hip_host_alloc / _free: the job level sits on include/dwgsim_hip.h and on nothing below it)
struct HostMem {
    void *p = nullptr; size_t cap = 0;
    HostMem() = default;
    HostMem(HostMem &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    HostMem &operator=(HostMem &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~HostMem() { dwgsim_hip_host_free(p); }
    // Room for `want` bytes with the first `keep` bytes kept.  Nothing to keep: the old block goes first, so that there are never two.
    // false: no memory -- what was to be kept still stands.
    bool grow(size_t want, size_t keep)
    {
        if (!keep) { dwgsim_hip_host_free(p); p = nullptr; cap = 0; }
        void *q = dwgsim_hip_host_alloc(want);
        if (!q) return false;
        if (p) { memcpy(q, p, keep); dwgsim_hip_host_free(p); }
        p = q; cap = want;
        return true;
    }
};
constexpr int JOB_STREAMS = 4;         // output streams of a batch: the three FASTQ streams and, with dwgsim_hip_job_set_truth_sam, DWGSIM_HIP_STREAM_SAM
struct PinBuf { HostMem s[JOB_STREAMS]; };      // the output of one batch, a block per stream

struct CtxDestroy { void operator()(dwgsim_hip_ctx_t *x) const { dwgsim_hip_destroy(x); } };
struct MutlistFree { void operator()(dwgsim_hip_mutlist_t *l) const { dwgsim_hip_mutlist_free(l); } };
using CtxPtr = std::unique_ptr<dwgsim_hip_ctx_t, CtxDestroy>;
using MutList = std::unique_ptr<dwgsim_hip_mutlist_t, MutlistFree>;

// One batch of a group, from the cut to the sink.  `ranges` and `pairs` are fixed at dispatch; every other field is guarded by the job's mutex.
struct Batch {
    std::vector<dwgsim_hip_range_t> ranges; uint64_t pairs = 0;      // contig = member ordinal (each device adds its own handle base)
    uint64_t rand_counted = 0, rand_got = 0;      // random reads: counted in advance by its device (k_place) / made by its kernels
    std::array<uint64_t, 4> fail_seg{{0, 0, 0, 0}};      // the abort rule's summary
    // the output, known when the batch's kernels are done (stage A): page-locked buffer (lent by device `lane`), bytes per stream as delivered and
    // as text, streams that still have to deliver it; ready = the copy-out has landed and the fields above are in (stage B)
    PinBuf *buf = nullptr; int lane = -1;
    uint64_t n[JOB_STREAMS] = {0, 0, 0, 0}, text_n[JOB_STREAMS] = {0, 0, 0, 0};
    int left = 0; bool ready = false;
    // reads_at (pieces with their place in the stream, delivered by several threads): sized = n[] is in; placed = so is n[] of every batch in
    // front of it, in file order across groups, and off[] is where its pieces go (assign_offsets)
    uint64_t off[JOB_STREAMS] = {0, 0, 0, 0}; bool sized = false, placed = false;
};

struct GroupJob {
    int id = 0;
    std::vector<std::string> names; std::vector<int64_t> lens, l_eff, n_pairs; std::vector<uint32_t> cindex;
    int stage_slot = -1; std::vector<const uint8_t *> ptrs;      // the sequence in page-locked staging, group layout
    int stage_users = 0;                                         // devices that have not walked it yet
    uint64_t pairs = 0;
    int nd = 1;                                                   // devices that share the group's batches: batch b belongs to device b mod nd
    std::vector<Batch> batch;
    int counted = 0;                                              // devices that have published their batches' counts
    bool base_known = false; uint64_t rand_base = 0;              // random reads in front of the group
    bool totalled = false;                                        // its total has been recorded (advance_rand_base)
    int batches_done = 0;
    int joined = 0; uint64_t fail_acc[4] = {0, 0, 0, 0};          // abort rule: batches 0 .. joined-1 are simulated and their summaries joined, in order
    // the truth VCF (dwgsim_hip_job_set_truth_vcf_sink): per contig the counters of the true read depth, summed over the devices that have handed theirs in
    // behind their last batch of the group (depth_in of them so far)
    std::vector<std::vector<uint64_t>> depth; int depth_in = 0;
};

// The pairs of a group's contigs, in file order, cut into read-index ranges: a multiple of nd near-equal batches of at most batch_pairs pairs, so
// that every device gets the same number of them, of the same size.  Pure arithmetic.
std::vector<Batch> cut_batches(const std::vector<int64_t> &n_pairs, int nd, uint64_t batch_pairs)
{
    std::vector<Batch> out;
    uint64_t pairs = 0; for (int64_t n : n_pairs) pairs += (uint64_t)n;
    if (!pairs) return out;
    const uint64_t nbt = (uint64_t)nd * ((pairs + (uint64_t)nd * batch_pairs - 1) / ((uint64_t)nd * batch_pairs));
    const uint64_t per = (pairs + nbt - 1) / nbt;
    Batch cur; uint64_t room = per;
    for (size_t k = 0; k < n_pairs.size(); ++k) {
        uint64_t first = 0, n = (uint64_t)n_pairs[k];
        while (n > 0) {
            const uint64_t take = n < room ? n : room;
            dwgsim_hip_range_t r; memset(&r, 0, sizeof r); r.contig = (int32_t)k; r.first_ii = first; r.n_pairs = take;
            cur.ranges.push_back(r); first += take; n -= take; room -= take; cur.pairs += take;
            if (room == 0) { out.push_back(cur); cur = Batch(); room = per; }
        }
    }
    if (!cur.ranges.empty()) out.push_back(cur);
    return out;
}

} // namespace

struct dwgsim_hip_job {
    // FIXED: written by job_create -- and, the contig table, regions and mutation input, by the set_ calls, which are refused once the threads
    // run -- and only read after that, by any thread.
    struct Fixed {
        dwgsim_hip_params_t prm; std::string prefix, flow;
        dwgsim_hip_job_sink_t sink; dwgsim_hip_job_options_t opt;
        std::vector<int> devices; std::vector<CtxPtr> ctx;
        int ND = 0;
        bool want_mut = true, want_reads = true, gzip = true;
        uint64_t batch_pairs = 1u << 18, group_bp = 32u << 20, min_share = 65536;      // (batches of 2^18 pairs: 190 MB of text, 94 MB of members -- measured against 2^17 .. 2^20: the smaller the batch, the shorter a job's fill and drain and the less page-locked memory there is to hand back; below 2^18 the whole-genome rate stops improving)
        int max_bufs = 8;      // page-locked output buffers per device (the batches in flight there, one per output set of the context, + what the delivery threads hold)
        bool tracing = false; double t0 = 0;
        // DWGSIM_HIP_SOLO=r/W (measurement only): the ONE device of this job does exactly what device r of a W-device job does -- walks every group it
        // takes part in, counts and simulates batches r, r + W, ... of each, copies them out, delivers them -- and nothing of the other devices' work.  The
        // path has no device-to-device traffic, so that is what device r's GPU and PCIe link would carry.  The other devices' batches are treated as
        // delivered and their random-read counts as zero (absent_devices_done): the OUTPUT of such a run is a share of the job with wrong rand_ii
        // offsets -- for a counting sink and a clock, not for files.  VD = devices the batches are dealt to (W, or ND), vrank(d) = which of them device d is.
        int solo_rank = -1, VD = 0;
        int vrank(int d) const { return solo_rank >= 0 ? solo_rank : d; }
        bool has_sink() const { return sink.reads != nullptr || sink.reads_at != nullptr; }
        // the contig table (dwgsim.c:465-478), -x and -m / -v
        std::vector<std::string> tab_names; std::vector<int64_t> tab_lens; bool have_table = false;
        uint64_t tot_len = 0;         // (start_threads: the regions' total once -x is in force)
        size_t stage_want = 0;        // room for the largest group, so that a staging buffer is page-locked once
        std::string regions_path, mutin_path; int mutin_type = -1;
        dwgsim_hip_job_haplotype_fn hap_fn = nullptr; void *hap_user = nullptr; int hap_width = 60;      // dwgsim_hip_job_set_haplotype_sink
        bool truth_sam = false;       // dwgsim_hip_job_set_truth_sam: every batch also delivers stream DWGSIM_HIP_STREAM_SAM
        bool truth_md = false;        // dwgsim_hip_job_set_truth_md: ... its mapped records with NM:i: and MD:Z:
        dwgsim_hip_job_truth_vcf_fn tvcf_fn = nullptr; void *tvcf_user = nullptr;      // dwgsim_hip_job_set_truth_vcf_sink
        dwgsim_hip_job_chain_fn chain_fn = nullptr; void *chain_user = nullptr;        // dwgsim_hip_job_set_chain_sink
    } cfg;

    // CALLER: touched only by the thread that calls the job_ functions (the ABI allows one at a time).  The workers see the staging through
    // the pointers a group carries from dispatch on, never through these.
    struct Caller {
        bool started = false, finished = false;
        int n_ref = 0; int64_t n_sim = 0; int prev_skip = 0; uint32_t next_index = 0;      // the scheduling state of the contig loop (dwgsim.c:519-625)
        static constexpr int N_STAGE = 2;      // (one being filled while the other's group is uploaded and walked; a third bought nothing and is 0.25 GB of page-locked memory for a genome)
        HostMem stage[N_STAGE];                // the sequence on its way to the devices
        uint8_t *stage_at(int s) const { return (uint8_t *)stage[s].p; }
        std::shared_ptr<GroupJob> pending; size_t pending_bytes = 0;           // the group being filled
        struct Open { bool open = false; std::string name; int64_t l = 0, st = 0, total = 0; uint32_t ci = 0; } open;      // the contig between begin_contig and commit_contig
        std::vector<std::thread> workers, deliverers;
    } me;

    // SHARED: guarded by m; cv is notified on every change another thread may be waiting for.  `failed` alone may be read without the lock.
    std::mutex m; std::condition_variable cv;
    std::atomic<bool> failed{false};
    struct Shared {
        std::string err;
        std::deque<std::shared_ptr<GroupJob>> groups;      // dispatched, not yet retired (front = oldest)
        int n_dispatched = 0; bool no_more = false;
        std::vector<int> next_group;                       // per device: id of the group it takes next
        bool stage_busy[Caller::N_STAGE] = {false, false};
        uint64_t next_off[JOB_STREAMS] = {0, 0, 0, 0}; int off_gid = 0, off_b = 0;      // reads_at: the next piece's offsets; the batch (group id, index) they belong to
        uint64_t delivered_pairs = 0;
        uint64_t total_rand = 0;                           // random reads up to the end of the last group that was totalled (advance_rand_base, its only writer)
        std::vector<std::vector<std::unique_ptr<PinBuf>>> bufs; std::vector<std::vector<PinBuf *>> free_bufs;      // page-locked output buffers per device: all / not lent
    } sh;

    // (the threads have been joined: job_finish.)  The contexts go first, as they always have; the members do the rest.
    ~dwgsim_hip_job() { cfg.ctx.clear(); }
};

namespace {

// DWGSIM_HIP_TRACE=1 (analysis): when the job's stages happen, in seconds since the job was created, on stderr
double mono_s() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
void trace(dwgsim_hip_job *j, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

void job_fail(dwgsim_hip_job *j, const std::string &what)
{
    std::lock_guard<std::mutex> g(j->m);
    if (!j->failed.exchange(true)) j->sh.err = what;
    j->cv.notify_all();
}

int arg_error(dwgsim_hip_job *j, int code, const char *what)      // a call that is refused: the text for last_error, the job itself goes on
{
    if (j) { std::lock_guard<std::mutex> g(j->m); if (!j->failed.load()) j->sh.err = what; }
    return code;
}

void say(dwgsim_hip_job *j, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void say(dwgsim_hip_job *j, const char *fmt, ...)
{
    char b[4608]; va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    if (j->cfg.sink.message) j->cfg.sink.message(j->cfg.sink.user, b); else if (!j->cfg.opt.quiet) fputs(b, stderr);
}

void trace(dwgsim_hip_job *j, const char *fmt, ...)
{
    if (!j->cfg.tracing) return;
    char b[256]; va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    fprintf(stderr, "[trace %8.4f] %s\n", mono_s() - j->cfg.t0, b);
}

std::shared_ptr<GroupJob> group_by_id(dwgsim_hip_job *j, int id)      // j->m held
{
    for (auto &g : j->sh.groups) if (g->id == id) return g;
    return nullptr;
}

// reads_at: offsets for every batch whose predecessors' sizes are all known (j->m held)
void assign_offsets(dwgsim_hip_job *j)
{
    if (!j->cfg.sink.reads_at) return;
    auto &sh = j->sh;
    for (;;) {
        auto g = group_by_id(j, sh.off_gid);
        if (!g) { if (sh.off_gid < sh.n_dispatched) { ++sh.off_gid; sh.off_b = 0; continue; } break; }      // (retired already: it had no batches)
        const int nb = (int)g->batch.size();
        for (; sh.off_b < nb && g->batch[(size_t)sh.off_b].sized; ++sh.off_b) {
            Batch &B = g->batch[(size_t)sh.off_b];
            for (int s = 0; s < JOB_STREAMS; ++s) { B.off[s] = sh.next_off[s]; sh.next_off[s] += B.n[s]; }
            B.placed = true;
        }
        if (sh.off_b < nb) break;
        ++sh.off_gid; sh.off_b = 0;
    }
}

// `pieces` streams of the batch have gone to the sink (0: it has just been published): behind the last one its buffer goes back to the device
// that lent it (j->m held)
void piece_delivered(dwgsim_hip_job *j, Batch &B, int pieces)
{
    B.left -= pieces;
    if (B.left == 0 && B.buf) { j->sh.free_bufs[(size_t)B.lane].push_back(B.buf); B.buf = nullptr; j->cv.notify_all(); }
}

// one user of the group's staging is done with it: behind the last one the buffer can be filled again (j->m held)
void release_stage(dwgsim_hip_job *j, GroupJob &g)
{
    if (--g.stage_users == 0) { j->sh.stage_busy[g.stage_slot] = false; j->cv.notify_all(); }
}

// The random-read chain (rand_ii, dwgsim.c:1042,1096), in this one place (j->m held).  A group is COMPLETE when the random reads of all its batches
// are known: with VD > 1 when every device that shares it has published its counts (count_mine; absent_devices_done for the devices of a solo run
// that are not there), with VD == 1 -- nothing is counted in advance, the device carries the count from batch to batch itself
// (DWGSIM_HIP_RAND_CHAIN) -- when its last batch has landed.  A complete group whose base is known gives the group behind it its base, if that
// group is there and has none.  Called by whoever may be the first to see that: a worker with the counts in (or passing a group by, or with the
// last batch landed), and dispatch for the group in front of the new one.
// total_rand has ONE writer, this function, once per group, the first time the group is seen complete.  A group's base comes from here or, at
// dispatch behind a retired group, from total_rand itself; so groups are totalled in order, total_rand never steps back, and when a group has
// retired -- all its batches made, which takes all its counts -- it is the total up to that group's end.
void advance_rand_base(dwgsim_hip_job *j, GroupJob &g)
{
    const bool complete = j->cfg.VD > 1 ? g.counted >= g.nd : g.batches_done >= (int)g.batch.size();
    if (!complete || !g.base_known) return;
    uint64_t tot = g.rand_base;
    for (const Batch &B : g.batch) tot += j->cfg.VD > 1 ? B.rand_counted : B.rand_got;
    if (!g.totalled) { j->sh.total_rand = tot; g.totalled = true; }
    auto nx = group_by_id(j, g.id + 1);
    if (nx && !nx->base_known) { nx->rand_base = tot; nx->base_known = true; j->cv.notify_all(); }
}

// ---- one device ----
struct Worker {
    dwgsim_hip_job *j; int d; dwgsim_hip_ctx_t *x;
    // A group on this device: its handle base, whether its walk has been waited for and whether this device has counted its random reads.
    // `ahead` is the NEXT group, as far as look_ahead() has got with it between two batches; process() adopts it whole.
    struct Resident { std::shared_ptr<GroupJob> g; int h = -1; bool walked = false, counted = false; };
    Resident ahead;
    bool first_batch_of_job = true;
    // The batches in flight, oldest first -- one per output set of the context, and they stay in flight ACROSS the end of a group: batch k is
    // enqueued (kernels); then the copy-out of batch k-1 is issued as soon as its kernels are done (stage A); then the copy-out of the oldest batch
    // is waited for and the batch published (stage B), which frees its slot for batch k+1.  With four slots two batches' copies are queued on the
    // copy stream while the worker does anything else, so the link does not wait for the host.  Rounds 3-4: two slots, the copy of a batch
    // issued only behind the enqueue of the next one (33 GB/s over a link that carries 54); round 5's first form: three slots, drained at every
    // group's end, where the worker then made the next group's mutation text -- 25 to 50 ms per chromosome during which the copy engine stood still
    // (profiles/r05_genome_trace.txt: busy 0.75).
    struct Pending { int slot = 0, b = 0, h = -1; bool a_done = false, last_of_group = false; std::shared_ptr<GroupJob> g; dwgsim_hip_batch_t bt; };
    std::deque<Pending> fl;
    uint64_t kk = 0;      // batches enqueued so far (batch kk takes slot kk mod DWGSIM_HIP_SLOTS)
    // (device 0) the mutation text: the worker only fetches a group's list of mutated cells; a thread of its own makes the text and hands it to the sink
    struct MutTask { MutList list; std::vector<std::string> names; };
    std::thread mut_thread; std::mutex mm; std::condition_variable mcv; std::deque<MutTask> mq; bool mut_quit = false;

    // (device 0) the haplotype FASTA (dwgsim_hip_job_set_haplotype_sink): behind a group's walk the worker has both texts made on the device -- two passes
    // over the cells on the walk stream -- and then copies them out piece by piece into a few page-locked buffers, BETWEEN the group's batches and only
    // while a buffer is free (pump_haplotypes), so that a slow sink holds up no batch; a thread of its own hands the pieces to the sink in order.  Only
    // before the group's memory goes back, or the next group's texts are made, does the worker wait for buffers.
    static constexpr size_t HAP_PIECE = (size_t)32 << 20; static constexpr int HAP_BUFS = 3;
    struct HapPiece { int hap; HostMem *buf; size_t len; };
    std::thread hap_thread; std::mutex hm; std::condition_variable hcv; std::deque<HapPiece> hq; bool hap_quit = false;
    std::vector<std::unique_ptr<HostMem>> hap_bufs; std::vector<HostMem *> hap_free;
    struct HapState { bool active = false; int h = -1, hap = 0; uint64_t off = 0, bytes[2] = {0, 0}; } hs;      // the group whose texts are on their way out

    // (device 0) the truth VCF: a second list of the group's mutated cells goes to a thread of its own, which waits until every device that simulates batches
    // of the group has handed its counters in (hand_depth_in, behind its last batch), then makes the records from their sum and hands them to the sink
    struct TvcfTask { MutList list; std::shared_ptr<GroupJob> g; };
    std::thread tvcf_thread; std::mutex tm; std::condition_variable tcv; std::deque<TvcfTask> tq; bool tvcf_quit = false;

    bool ok() const { return !j->failed.load(); }
    void fail_ctx() { job_fail(j, std::string("dwgsim-hip: ") + dwgsim_hip_last_error(x)); }
    bool mine(const GroupJob &g, int b) const { return b % g.nd == j->cfg.vrank(d); }
    bool takes_part(const GroupJob &g) const { return j->cfg.vrank(d) == 0 || (j->cfg.want_reads && j->cfg.vrank(d) < g.nd); }      // device 0 also writes the mutation text

    void mut_loop()      // mut_print (mut.c:781-893), groups and contigs in order
    {
        const auto &sink = j->cfg.sink;
        for (;;) {
            MutTask t;
            {
                std::unique_lock<std::mutex> lk(mm);
                mcv.wait(lk, [&]() { return mut_quit || !mq.empty(); });
                if (mq.empty()) return;
                t = std::move(mq.front()); mq.pop_front();
            }
            for (size_t k = 0; k < t.names.size() && ok(); ++k) {
                const char *tx, *v; size_t tl, vl;
                if (dwgsim_hip_mutlist_text(t.list.get(), (int)k, &tx, &tl, &v, &vl) < 0) { job_fail(j, "dwgsim-hip: the mutation text could not be made"); break; }
                if (sink.mutations(sink.user, t.names[k].c_str(), tx, tl, v, vl) != 0) { job_fail(j, "dwgsim-hip: the sink refused the mutation text"); break; }
            }
        }
    }
    void mut_stop()
    {
        if (!mut_thread.joinable()) return;
        { std::lock_guard<std::mutex> lk(mm); mut_quit = true; }
        mcv.notify_all();
        mut_thread.join();
    }

    // devices of this job that simulate batches of the group, and so hand counters in
    int depth_devices(const GroupJob &g) const
    {
        int n = 0;
        for (int dd = 0; dd < j->cfg.ND; ++dd) { bool any = false; for (int b = 0; b < (int)g.batch.size(); ++b) if (b % g.nd == j->cfg.vrank(dd)) any = true; n += any ? 1 : 0; }
        return n;
    }
    void tvcf_loop()      // groups and contigs in order
    {
        for (;;) {
            TvcfTask t;
            {
                std::unique_lock<std::mutex> lk(tm);
                tcv.wait(lk, [&]() { return tvcf_quit || !tq.empty(); });
                if (tq.empty()) return;
                t = std::move(tq.front()); tq.pop_front();
            }
            std::vector<std::vector<uint64_t>> sum;
            {
                std::unique_lock<std::mutex> lk(j->m);
                const int want = depth_devices(*t.g);
                j->cv.wait(lk, [&]() { return j->failed.load() || t.g->depth_in >= want; });
                sum.swap(t.g->depth);
            }
            for (size_t k = 0; k < t.g->names.size() && ok(); ++k) {
                const char *v; size_t vl;
                const bool have = k < sum.size() && !sum[k].empty();      // (no device simulated anything of the group: every depth is 0)
                if (dwgsim_hip_mutlist_truth_vcf_text(t.list.get(), (int)k, have ? sum[k].data() : nullptr, have ? sum[k].size() / 2 : 0, &v, &vl) < 0) { job_fail(j, "dwgsim-hip: the truth VCF could not be made"); break; }
                if (j->cfg.tvcf_fn(j->cfg.tvcf_user, t.g->names[k].c_str(), v, vl) != 0) { job_fail(j, "dwgsim-hip: the sink refused the truth VCF"); break; }
            }
        }
    }
    void tvcf_stop()
    {
        if (!tvcf_thread.joinable()) return;
        { std::lock_guard<std::mutex> lk(tm); tvcf_quit = true; }
        tcv.notify_all();
        tvcf_thread.join();
    }
    // this device's last batch of the group is done: its counters of the true read depth, contig by contig, are added to the group's
    bool hand_depth_in(GroupJob &g, int h)
    {
        const size_t n = g.names.size();
        std::vector<std::vector<uint64_t>> mine(n);
        for (size_t k = 0; k < n; ++k) {
            const int64_t cells = dwgsim_hip_truth_depth_fetch(x, h + (int)k, nullptr, 0);
            if (cells < 0) { fail_ctx(); return false; }
            mine[k].assign(2 * (size_t)cells, 0);
            if (cells && dwgsim_hip_truth_depth_fetch(x, h + (int)k, mine[k].data(), (size_t)cells) != cells) { fail_ctx(); return false; }
        }
        std::lock_guard<std::mutex> lk(j->m);
        if (g.depth.empty()) g.depth.swap(mine);
        else for (size_t k = 0; k < n; ++k) {
            if (g.depth[k].size() != mine[k].size()) { if (!j->failed.exchange(true)) j->sh.err = "dwgsim-hip: two devices list different mutated cells for one contig"; j->cv.notify_all(); return false; }
            for (size_t q = 0; q < mine[k].size(); ++q) g.depth[k][q] += mine[k][q];
        }
        ++g.depth_in;
        j->cv.notify_all();
        return true;
    }

    void hap_loop()      // the pieces in the order the worker made them: each haplotype's file in order
    {
        for (;;) {
            HapPiece t;
            {
                std::unique_lock<std::mutex> lk(hm);
                hcv.wait(lk, [&]() { return hap_quit || !hq.empty(); });
                if (hq.empty()) return;
                t = hq.front(); hq.pop_front();
            }
            if (ok() && j->cfg.hap_fn(j->cfg.hap_user, t.hap, t.buf->p, t.len) != 0) job_fail(j, "dwgsim-hip: the sink refused the haplotype text");
            { std::lock_guard<std::mutex> lk(hm); hap_free.push_back(t.buf); }
            hcv.notify_all();
        }
    }
    void hap_stop()
    {
        if (!hap_thread.joinable()) return;
        { std::lock_guard<std::mutex> lk(hm); hap_quit = true; }
        hcv.notify_all();
        hap_thread.join();
    }
    // a page-locked buffer for the next piece; wait = false: nullptr when none is free
    HostMem *hap_take_buf(bool wait)
    {
        std::unique_lock<std::mutex> lk(hm);
        if (hap_free.empty() && (int)hap_bufs.size() < HAP_BUFS) { hap_bufs.push_back(std::make_unique<HostMem>()); hap_free.push_back(hap_bufs.back().get()); }
        if (hap_free.empty() && wait) hcv.wait(lk, [&]() { return !hap_free.empty() || !ok(); });
        if (hap_free.empty()) return nullptr;
        HostMem *b = hap_free.back(); hap_free.pop_back();
        return b;
    }
    // as many pieces of the current group's texts as there are free buffers (wait: all that is left of them); false: the job has failed
    bool pump_haplotypes(bool wait)
    {
        while (hs.active) {
            if (!ok()) return false;
            if (hs.off >= hs.bytes[hs.hap]) { hs.off = 0; if (++hs.hap == 2) hs.active = false; continue; }
            HostMem *b = hap_take_buf(wait);
            if (!b) return ok() && !wait;
            const uint64_t left = hs.bytes[hs.hap] - hs.off;
            const size_t len = left < HAP_PIECE ? (size_t)left : HAP_PIECE;
            bool fine = b->cap >= len || b->grow(len <= ((size_t)1 << 20) ? (size_t)1 << 20 : HAP_PIECE, 0);
            if (!fine) job_fail(j, "dwgsim-hip: cannot allocate page-locked host memory for the haplotype text");
            else if (dwgsim_hip_haplotype_fetch(x, hs.hap, hs.off, b->p, len) < 0) { fail_ctx(); fine = false; }
            if (!fine) { std::lock_guard<std::mutex> lk(hm); hap_free.push_back(b); return false; }
            { std::lock_guard<std::mutex> lk(hm); hq.push_back(HapPiece{hs.hap, b, len}); }
            hcv.notify_all();
            hs.off += len;
        }
        return true;
    }
    // the group's memory is about to go back: what is left of its texts goes out first
    bool flush_haplotypes(int h) { return !(hs.active && hs.h == h) || pump_haplotypes(true); }

    int prep(const std::shared_ptr<GroupJob> &g)      // upload (asynchronous: the staging is page-locked and in group layout) and enqueue the walk
    {
        const int n = (int)g->names.size();
        std::vector<const char *> nm((size_t)n);
        for (int k = 0; k < n; ++k) nm[(size_t)k] = g->names[(size_t)k].c_str();
        const int h = dwgsim_hip_add_contigs(x, n, nm.data(), g->ptrs.data(), g->lens.data(), g->cindex.data());
        if (h < 0) { fail_ctx(); return -1; }
        if (!j->cfg.regions_path.empty())      // the `l` of fragment placement: the region length -- or the full length for the last contig of an -N run (dwgsim.c:535-537)
            for (int k = 0; k < n; ++k) if (dwgsim_hip_contig_set_placement_length(x, h + k, g->l_eff[(size_t)k]) < 0) { fail_ctx(); return -1; }
        if (dwgsim_hip_mutate_async(x, h) < 0) { fail_ctx(); return -1; }
        return h;
    }

    // the walk has finished: the staging is no longer needed by this device
    bool walked(Resident &r)
    {
        if (dwgsim_hip_mutate_wait(x, r.h) < 0) { fail_ctx(); return false; }
        r.walked = true;
        std::lock_guard<std::mutex> lk(j->m);
        release_stage(j, *r.g);
        return true;
    }

    // random reads of my batches of the group, counted without producing them (k_place on the walk stream): one launch, one count per batch
    bool count_mine(Resident &r)
    {
        GroupJob &g = *r.g;
        r.counted = true;
        if (j->cfg.vrank(d) >= g.nd) return true;
        std::vector<dwgsim_hip_range_t> all; std::vector<int> owner;
        for (int b = 0; b < (int)g.batch.size(); ++b) if (mine(g, b)) for (auto q : g.batch[(size_t)b].ranges) { q.contig += r.h; all.push_back(q); owner.push_back(b); }
        std::vector<uint64_t> per(all.size(), 0); uint64_t tot = 0;
        if (!all.empty() && dwgsim_hip_count_random_ranges(x, all.data(), (int)all.size(), &tot, per.data()) < 0) { fail_ctx(); return false; }
        std::lock_guard<std::mutex> lk(j->m);
        for (size_t q = 0; q < all.size(); ++q) g.batch[(size_t)owner[q]].rand_counted += per[q];
        ++g.counted;
        j->cv.notify_all();
        return true;
    }

    // between two batches: whatever can be done for the NEXT group without waiting -- upload + walk as soon as it has been handed over, the count
    // of its random reads as soon as its walk has finished -- so that its first batch follows this group's last one at once
    bool look_ahead(const GroupJob &g)
    {
        if (!ahead.g) {
            std::shared_ptr<GroupJob> nx;
            { std::lock_guard<std::mutex> lk(j->m); nx = group_by_id(j, g.id + 1); }
            if (nx && takes_part(*nx)) { const int nh = prep(nx); if (nh < 0) return false; ahead = Resident{nx, nh}; }
        }
        if (ahead.g && !ahead.walked && dwgsim_hip_mutate_poll(x, ahead.h) == 1 && !walked(ahead)) return false;
        if (ahead.g && ahead.walked && !ahead.counted && j->cfg.VD > 1 && j->cfg.want_reads && !count_mine(ahead)) return false;
        return true;
    }

    PinBuf *acquire(const uint64_t need[JOB_STREAMS])
    {
        PinBuf *b = nullptr;
        {
            std::unique_lock<std::mutex> lk(j->m);
            auto &fr = j->sh.free_bufs[(size_t)d]; auto &all = j->sh.bufs[(size_t)d];
            j->cv.wait(lk, [&]() { return !fr.empty() || (int)all.size() < j->cfg.max_bufs || j->failed.load(); });
            if (j->failed.load()) return nullptr;
            if (!fr.empty()) { b = fr.back(); fr.pop_back(); }
            else { all.push_back(std::make_unique<PinBuf>()); b = all.back().get(); }
        }
        for (int s = 0; s < JOB_STREAMS; ++s)
            if (need[s] > b->s[s].cap && !b->s[s].grow((size_t)need[s] + (size_t)need[s] / 8 + 4096, 0)) { job_fail(j, "dwgsim-hip: cannot allocate page-locked host memory for the output"); return nullptr; }
        return b;
    }

    // stage A: the batch's kernels are done -- its sizes are known: the copy-out is issued; the last batch of a group also gives the group's memory back
    bool stage_a(Pending &pb)
    {
        if (pb.a_done) return true;
        if (dwgsim_hip_wait(x, pb.slot, &pb.bt) < 0) { fail_ctx(); return false; }
        pb.a_done = true;
        uint64_t n[JOB_STREAMS], text_n[JOB_STREAMS];      // bytes per stream as delivered / as text (the truth SAM: 0 unless switched on)
        for (int s = 0; s < 3; ++s) { n[s] = j->cfg.gzip ? pb.bt.gz_bytes[s] : pb.bt.bytes[s]; text_n[s] = pb.bt.bytes[s]; }
        n[DWGSIM_HIP_STREAM_SAM] = j->cfg.gzip ? pb.bt.sam_gz_bytes : pb.bt.sam_bytes; text_n[DWGSIM_HIP_STREAM_SAM] = pb.bt.sam_bytes;
        if (j->cfg.has_sink()) {
            PinBuf *tb = acquire(n);
            if (!tb) return false;
            int left = 0;
            for (int s = 0; s < JOB_STREAMS; ++s) if (n[s]) {
                char *to = (char *)tb->s[s].p; const size_t cap = tb->s[s].cap;
                if ((j->cfg.gzip ? dwgsim_hip_fetch_gz_async(x, pb.slot, s, to, cap) : dwgsim_hip_fetch_async(x, pb.slot, s, to, cap)) < 0) { fail_ctx(); return false; }
                ++left;
            }
            std::lock_guard<std::mutex> lk(j->m);
            Batch &B = pb.g->batch[(size_t)pb.b];
            B.buf = tb; B.lane = d; B.left = left;
            for (int s = 0; s < JOB_STREAMS; ++s) { B.n[s] = n[s]; B.text_n[s] = text_n[s]; }
            if (j->cfg.sink.reads_at) { B.sized = true; assign_offsets(j); j->cv.notify_all(); }      // this batch's offsets, and those of any batch behind it that was only waiting for its sizes
        }
        if (pb.b < 2 * j->cfg.VD) trace(j, "dev %d group %d: batch %d kernels done, copy issued (%.1f MB)", d, pb.g->id, pb.b, j->cfg.has_sink() ? (n[0] + n[1] + n[2] + n[3]) / 1e6 : 0.0);
        if (pb.last_of_group && j->cfg.tvcf_fn && !hand_depth_in(*pb.g, pb.h)) return false;      // (every batch of the group on this device is done: they run in order on one stream)
        if (pb.last_of_group && !flush_haplotypes(pb.h)) return false;
        if (pb.last_of_group && dwgsim_hip_drop_contig(x, pb.h) < 0) { fail_ctx(); return false; }      // (the kernels of the group's last batch are done: nothing reads it any more)
        return true;
    }
    // stage B: the copy-out has landed: the batch is published (the delivery threads hand it to the sink in file order, behind the abort rule's verdict)
    bool stage_b(Pending &pb)
    {
        if (j->cfg.has_sink() && dwgsim_hip_fetch_wait(x, pb.slot) < 0) { fail_ctx(); return false; }
        if (pb.b < 2 * j->cfg.VD) trace(j, "dev %d group %d: batch %d landed", d, pb.g->id, pb.b);
        GroupJob &g = *pb.g; const int nb = (int)g.batch.size();
        uint64_t shown = 0; bool aborted = false;
        {
            std::lock_guard<std::mutex> lk(j->m);
            Batch &B = g.batch[(size_t)pb.b];
            for (int q = 0; q < 4; ++q) B.fail_seg[(size_t)q] = pb.bt.fail_seg[q];
            B.rand_got = pb.bt.n_random;
            B.ready = true;
            piece_delivered(j, B, 0);      // (no stream has anything of it: the buffer goes back at once)
            if (++g.batches_done == nb && j->cfg.VD == 1) advance_rand_base(j, g);
            // the abort rule (dwgsim.c:635, :833-843) over the batches of several devices: the summaries are joined in read-index order as soon
            // as the batches in front are complete -- a batch goes to the sink only behind its verdict (deliver_loop waits for `joined`)
            while (!aborted && g.joined < nb && g.batch[(size_t)g.joined].ready) {
                if (dwgsim_hip_failseg_join(g.fail_acc, g.batch[(size_t)g.joined].fail_seg.data())) aborted = true; else ++g.joined;
            }
            shown = (j->sh.delivered_pairs += pb.bt.n_pairs);
            j->cv.notify_all();
        }
        if (aborted) { job_fail(j, "\r[dwgsim_core] failed to generate a read after 10001 trials\n"); return false; }
        if (!j->cfg.opt.quiet) say(j, "\r[dwgsim_core] %llu", (unsigned long long)shown);      // (outside the lock: a sink may call back into the job)
        return true;
    }
    // everything in flight goes through both stages (before the worker waits for anything another thread can only provide once these batches are published)
    bool drain()
    {
        while (!fl.empty()) {
            for (auto &pb : fl) if (!stage_a(pb)) return false;
            if (!stage_b(fl.front())) return false;
            fl.pop_front();
        }
        return true;
    }
    // the job has failed: leave the context idle -- kernels and copies of whatever is in flight are waited for, nothing more is published
    void abandon()
    {
        for (auto &pb : fl) { if (!pb.a_done) { dwgsim_hip_batch_t bt; (void)dwgsim_hip_wait(x, pb.slot, &bt); } (void)dwgsim_hip_fetch_wait(x, pb.slot); }
        fl.clear();
    }

    void run()
    {
        pin_thread_to_device_node(j->cfg.devices[(size_t)d]);
        if (j->cfg.vrank(d) == 0 && j->cfg.want_mut && j->cfg.sink.mutations) mut_thread = std::thread([this]() { mut_loop(); });
        if (j->cfg.vrank(d) == 0 && j->cfg.hap_fn) hap_thread = std::thread([this]() { hap_loop(); });
        if (j->cfg.vrank(d) == 0 && j->cfg.tvcf_fn) tvcf_thread = std::thread([this]() { tvcf_loop(); });
        bool fine = true;
        for (;;) {
            std::shared_ptr<GroupJob> g;
            {
                std::unique_lock<std::mutex> lk(j->m);
                const int want = j->sh.next_group[(size_t)d];
                auto there = [&]() { return j->failed.load() || group_by_id(j, want) || (j->sh.no_more && want >= j->sh.n_dispatched); };
                if (!there() && !fl.empty()) {      // the next group may only be handed over once the one in front has retired -- which takes the batches still in flight here
                    lk.unlock();
                    if (!drain()) { fine = false; break; }
                    lk.lock();
                }
                j->cv.wait(lk, there);
                if (j->failed.load()) { fine = false; break; }
                g = group_by_id(j, want);
                if (!g) break;
                j->sh.next_group[(size_t)d] = want + 1;
            }
            if (!process(g)) { fine = false; break; }
        }
        if (fine && ok()) fine = drain();
        if (!fine || !ok()) abandon();
        if (ahead.g && !ahead.walked) (void)dwgsim_hip_mutate_wait(x, ahead.h);
        mut_stop();
        hap_stop();
        tvcf_stop();
    }

    // ---- one group: process() and its steps ----
    bool process(const std::shared_ptr<GroupJob> &g)
    {
        if (!takes_part(*g)) return pass_by(*g);      // a small group is not worth a copy on every device
        Resident cur;
        return adopt_or_prepare(g, cur) && hand_mutations_on(cur) && hand_haplotypes_on(cur) && hand_chains_on(cur) && exchange_counts(cur) && run_batches(cur);
    }

    bool pass_by(GroupJob &g)
    {
        std::lock_guard<std::mutex> lk(j->m);
        advance_rand_base(j, g);      // (a solo run: the device that would do this for the group is not there)
        release_stage(j, g);
        j->cv.notify_all();
        return true;
    }

    // the group is resident and walked: taken over from the look-ahead, or uploaded and walked now
    bool adopt_or_prepare(const std::shared_ptr<GroupJob> &g, Resident &cur)
    {
        if (ahead.g && ahead.g->id == g->id) { cur = std::move(ahead); ahead = Resident(); }
        else {
            trace(j, "dev %d group %d: prep", d, g->id);
            cur.g = g;
            if ((cur.h = prep(g)) < 0) return false;
            trace(j, "dev %d group %d: upload + walk enqueued", d, g->id);
        }
        if (!cur.walked && !walked(cur)) return false;
        trace(j, "dev %d group %d: walked", d, g->id);
        return true;
    }

    // (device 0) the group's list of mutated cells goes to the text thread (a few MB; the device part takes well under a millisecond)
    bool hand_mutations_on(const Resident &cur)
    {
        if (tvcf_thread.joinable()) {      // the truth VCF takes a list of its own: its thread makes the text when the group's last batch is done, long after the mutation text
            int n = 0;
            MutList L(dwgsim_hip_mutations_take(x, cur.h, &n));
            if (!L) { fail_ctx(); return false; }
            { std::lock_guard<std::mutex> lk(tm); tq.push_back(TvcfTask{std::move(L), cur.g}); }
            tcv.notify_all();
        }
        if (!mut_thread.joinable()) return true;
        int n = 0;
        MutList L(dwgsim_hip_mutations_take(x, cur.h, &n));
        if (!L) { fail_ctx(); return false; }
        { std::lock_guard<std::mutex> lk(mm); mq.push_back(MutTask{std::move(L), cur.g->names}); }
        mcv.notify_all();
        trace(j, "dev %d group %d: mutation list taken", d, cur.g->id);
        return true;
    }

    // (device 0) both haplotypes' FASTA text is made on the device now -- before the next group's walk is enqueued on the same stream -- and starts to go out
    bool hand_haplotypes_on(const Resident &cur)
    {
        if (!hap_thread.joinable()) return true;
        if (!pump_haplotypes(true)) return false;      // (what is left of the group in front, whose last batches may still be in flight: haplotype_fetch reads the text made last)
        hs = HapState(); hs.h = cur.h;
        for (int hap = 0; hap < 2; ++hap) if (dwgsim_hip_haplotype_fasta(x, cur.h, hap, j->cfg.hap_width, &hs.bytes[hap]) < 0) { fail_ctx(); return false; }
        hs.active = true;
        trace(j, "dev %d group %d: haplotype text made (%.1f MB)", d, cur.g->id, (hs.bytes[0] + hs.bytes[1]) / 1e6);
        return pump_haplotypes(false);
    }

    // (device 0) the chains of both haplotypes: two passes over the cells on the device, a few bytes per block to the host, the text made here and handed to the
    // sink by this thread -- a file's pieces in file order, a few megabytes for a whole genome
    uint64_t chain_next_id[2] = {1, 1};      // the id of a haplotype's next chain (its two directions carry the same ids)
    bool hand_chains_on(const Resident &cur)
    {
        if (j->cfg.vrank(d) != 0 || !j->cfg.chain_fn) return true;
        const GroupJob &g = *cur.g;
        std::vector<dwgsim_hip_chain_block_t> blk;
        std::string text[2];      // DWGSIM_HIP_CHAIN_TO_REF, _FROM_REF
        for (int hap = 0; hap < 2; ++hap) {
            if (dwgsim_hip_haplotype_chain(x, cur.h, hap, nullptr) < 0) { fail_ctx(); return false; }
            text[0].clear(); text[1].clear();
            for (size_t k = 0; k < g.names.size(); ++k) {
                uint64_t n = 0; int64_t ref_start = 0;
                if (dwgsim_hip_chain_blocks(x, cur.h + (int)k, hap, &n, nullptr, nullptr, 0) < 0) { fail_ctx(); return false; }
                if (n == 0) continue;      // (every cell deleted: no chain)
                blk.resize((size_t)n);
                if (dwgsim_hip_chain_blocks(x, cur.h + (int)k, hap, nullptr, &ref_start, blk.data(), n) < 0) { fail_ctx(); return false; }
                for (int dir = 0; dir < 2; ++dir) {
                    const int64_t need = dwgsim_hip_chain_format(g.names[k].c_str(), g.lens[k], ref_start, blk.data(), n, dir, chain_next_id[hap], nullptr, 0);
                    if (need < 0) { job_fail(j, "dwgsim-hip: the blocks of contig '" + g.names[k] + "' make no chain"); return false; }
                    const size_t at = text[dir].size();
                    text[dir].resize(at + (size_t)need);
                    (void)dwgsim_hip_chain_format(g.names[k].c_str(), g.lens[k], ref_start, blk.data(), n, dir, chain_next_id[hap], &text[dir][at], (size_t)need);
                }
                ++chain_next_id[hap];
            }
            for (int dir = 0; dir < 2; ++dir)
                if (!text[dir].empty() && j->cfg.chain_fn(j->cfg.chain_user, hap, dir, text[dir].data(), text[dir].size()) != 0) { job_fail(j, "dwgsim-hip: the sink refused the chain text"); return false; }
        }
        trace(j, "dev %d group %d: chains made", d, g.id);
        return true;
    }

    // several devices: my batches' random reads are counted and published; then every device's counts, and the group's base, are waited for
    bool exchange_counts(Resident &cur)
    {
        if (j->cfg.VD == 1 || !j->cfg.want_reads) return true;
        if (!cur.counted && !count_mine(cur)) return false;
        GroupJob &g = *cur.g;
        std::unique_lock<std::mutex> lk(j->m);
        auto counts_in = [&]() { return j->failed.load() || (g.counted >= g.nd && g.base_known); };
        if (!counts_in() && !fl.empty()) {      // another device may be waiting for page-locked buffers that only come back once the batches in flight here are published
            lk.unlock();
            if (!drain()) return false;
            lk.lock();
        }
        j->cv.wait(lk, counts_in);
        if (j->failed.load()) return false;
        advance_rand_base(j, g);      // (every device computes the same thing; the first one publishes it for the next group)
        return true;
    }

    // my batches of the group, two to three in flight, with the look-ahead between them
    bool run_batches(const Resident &cur)
    {
        GroupJob &g = *cur.g; const int h = cur.h;
        std::vector<int> todo;
        for (int b = 0; b < (int)g.batch.size(); ++b) if (mine(g, b)) todo.push_back(b);
        if (todo.empty()) {      // nothing to simulate here (device 0 of a small group, or -o 2): the group's memory goes back at once
            if (!flush_haplotypes(h)) return false;
            if (dwgsim_hip_drop_contig(x, h) < 0) { fail_ctx(); return false; }
            return look_ahead(g);
        }
        // the next group, if it is already here, is uploaded and walked on the walk stream while this one's batches run
        if (!look_ahead(g)) return false;
        for (size_t q = 0; q < todo.size(); ++q) {
            const int b = todo[q];
            if (!ok()) return false;
            uint64_t rbase;
            if (j->cfg.VD > 1) { rbase = g.rand_base; for (int t = 0; t < b; ++t) rbase += g.batch[(size_t)t].rand_counted; }      // (final: all devices have published)
            else { rbase = first_batch_of_job ? 0 : DWGSIM_HIP_RAND_CHAIN; first_batch_of_job = false; }
            std::vector<dwgsim_hip_range_t> r = g.batch[(size_t)b].ranges;
            for (auto &t : r) t.contig += h;
            const int slot = (int)(kk % DWGSIM_HIP_SLOTS);      // (free: at most DWGSIM_HIP_SLOTS - 1 batches are in flight here)
            if (dwgsim_hip_simulate_ranges_async(x, r.data(), (int)r.size(), rbase, slot) < 0) { fail_ctx(); return false; }
            if (q < 3 || q + 1 == todo.size()) trace(j, "dev %d group %d: batch %d enqueued", d, g.id, b);
            ++kk;
            fl.emplace_back();
            Pending &pb = fl.back(); pb.slot = slot; pb.b = b; pb.h = h; pb.g = cur.g; pb.last_of_group = q + 1 == todo.size();
            for (size_t t = 0; t + 1 < fl.size(); ++t) if (!stage_a(fl[t])) return false;
            while ((int)fl.size() >= DWGSIM_HIP_SLOTS) { if (!stage_b(fl.front())) return false; fl.pop_front(); }
            if (!pump_haplotypes(false)) return false;
            if (!look_ahead(g)) return false;
        }
        return ok();
    }
};

// One delivery thread: stream s of every batch in file order, handed to sink.reads (dev < 0: one thread per stream) -- or stream s of the batches
// device `dev` made, each piece with its offset, handed to sink.reads_at (one thread per device and stream: N devices deliver side by side, where
// the ordered form's one thread per stream carries 21-26 GB/s through a sink that touches the bytes: profiles/r06_solo_rank_entry.txt -- below
// one device's link).  The two differ in which batches they visit, in what they wait for, and in the call.
void deliver_loop(dwgsim_hip_job *j, int dev, int s)
{
    const auto &sink = j->cfg.sink; const int gz = j->cfg.gzip ? 1 : 0;
    for (int gid = 0;; ++gid) {
        std::shared_ptr<GroupJob> g;
        {
            std::unique_lock<std::mutex> lk(j->m);
            j->cv.wait(lk, [&]() { return j->failed.load() || gid < j->sh.n_dispatched || j->sh.no_more; });
            if (j->failed.load() || gid >= j->sh.n_dispatched) return;
            g = group_by_id(j, gid);
            if (!g) continue;      // retired already: it had nothing for this thread
        }
        for (int b = 0; b < (int)g->batch.size(); ++b) {
            if (dev >= 0 && b % g->nd != j->cfg.vrank(dev)) continue;
            Batch &B = g->batch[(size_t)b];
            const char *p; uint64_t n, text_n, off;
            {
                std::unique_lock<std::mutex> lk(j->m);
                // simulated, landed and behind the abort rule's verdict over everything up to it; reads_at: and placed
                j->cv.wait(lk, [&]() { return j->failed.load() || (g->joined > b && (dev < 0 || B.placed)); });
                if (j->failed.load()) return;
                n = B.n[s]; text_n = B.text_n[s]; off = B.off[s]; p = n ? (const char *)B.buf->s[s].p : nullptr;
            }
            if (!n) continue;      // (nothing of it in this stream; a solo run: another device's batch, not made here)
            if ((dev < 0 ? sink.reads(sink.user, s, p, n, text_n, gz) : sink.reads_at(sink.user, s, off, p, n, text_n, gz)) != 0) { job_fail(j, "dwgsim-hip: writing FASTQ failed"); return; }
            std::lock_guard<std::mutex> lk(j->m);
            piece_delivered(j, B, 1);
        }
    }
}

// the group is complete when every batch was simulated (stage_b has joined the abort rule's summaries by then) and delivered: retire it
void retire_loop_step(dwgsim_hip_job *j)      // j->m held
{
    while (!j->sh.groups.empty()) {
        GroupJob &g = *j->sh.groups.front();
        const int nb = (int)g.batch.size();
        bool delivered = g.batches_done >= nb && g.joined >= nb;
        for (int b = 0; b < nb && delivered; ++b) if (!g.batch[(size_t)b].ready || g.batch[(size_t)b].left > 0) delivered = false;
        bool all_taken = true;
        for (int d = 0; d < j->cfg.ND; ++d) if (j->sh.next_group[(size_t)d] <= g.id) all_taken = false;
        if (!delivered || !all_taken || g.stage_users > 0) break;
        j->sh.groups.pop_front();
    }
}

// ---- dispatch: the group that was being filled goes to the devices ----

// where the group's sequences stand in the staging as it is now (begin_contig may have moved it after earlier commits, also for a contig that was then skipped)
void resolve_staging(dwgsim_hip_job *j, GroupJob &g)
{
    std::vector<int64_t> starts(g.lens.size());
    (void)dwgsim_hip_group_layout(g.lens.data(), (int)g.lens.size(), starts.data());
    g.ptrs.clear();
    for (size_t k = 0; k < g.lens.size(); ++k) g.ptrs.push_back(j->me.stage_at(g.stage_slot) + starts[k]);
}

// DWGSIM_HIP_SOLO: the devices that are not there.  Their batches count as simulated, joined (their abort-rule summaries are the identity), sized
// (nothing) and delivered; their random-read counts as published, and zero -- what is left to count is this device's own share, if it has one.
void absent_devices_done(const dwgsim_hip_job *j, GroupJob &g)
{
    if (j->cfg.solo_rank < 0) return;
    for (size_t b = 0; b < g.batch.size(); ++b) if ((int)(b % (size_t)g.nd) != j->cfg.solo_rank) { g.batch[b].ready = g.batch[b].sized = true; ++g.batches_done; }
    while (g.joined < (int)g.batch.size() && g.batch[(size_t)g.joined].ready) ++g.joined;
    const bool counts_here = j->cfg.VD > 1 && j->cfg.want_reads && j->cfg.solo_rank < g.nd;
    g.counted = g.nd - (counts_here ? 1 : 0);
}

// the hand-over: at most two groups in front of the devices (the staging of a third one is being filled meanwhile); the group gets its id and,
// where that is already known, the random reads in front of it
int hand_over(dwgsim_hip_job *j, const std::shared_ptr<GroupJob> &g)
{
    std::unique_lock<std::mutex> lk(j->m);
    j->cv.wait(lk, [&]() { retire_loop_step(j); return j->failed.load() || j->sh.groups.size() < 2; });
    if (j->failed.load()) return DWGSIM_HIP_ERR_FAILED;
    g->id = j->sh.n_dispatched++;
    auto front = group_by_id(j, g->id - 1);
    if (g->id == 0 || !front) { g->rand_base = j->sh.total_rand; g->base_known = true; }      // the first group (0), or the group in front has retired: its total is final
    j->sh.groups.push_back(g);
    if (front) advance_rand_base(j, *front);      // (if it is complete already; else whoever completes it hands the base on)
    assign_offsets(j);
    j->cv.notify_all();
    return DWGSIM_HIP_OK;
}

int dispatch_pending(dwgsim_hip_job *j)
{
    if (!j->me.pending) return DWGSIM_HIP_OK;
    auto g = std::move(j->me.pending); j->me.pending_bytes = 0;
    if (g->names.empty()) {      // every contig that was begun for it was skipped: only the staging goes back
        std::lock_guard<std::mutex> lk(j->m);
        g->stage_users = 1; release_stage(j, *g);
        return DWGSIM_HIP_OK;
    }
    resolve_staging(j, *g);
    for (int64_t n : g->n_pairs) g->pairs += (uint64_t)n;
    for (g->nd = j->cfg.VD; g->nd > 1 && g->pairs / (uint64_t)g->nd < j->cfg.min_share;) --g->nd;      // a device's share of a small group is not worth its walk
    if (j->cfg.want_reads) g->batch = cut_batches(g->n_pairs, g->nd, j->cfg.batch_pairs);
    absent_devices_done(j, *g);
    g->stage_users = j->cfg.ND;
    const int rc = hand_over(j, g);
    if (rc == DWGSIM_HIP_OK) trace(j, "group %d dispatched (%zu contigs, %llu pairs, %zu batches)", g->id, g->names.size(), (unsigned long long)g->pairs, g->batch.size());
    return rc;
}

int start_threads(dwgsim_hip_job *j)
{
    if (j->me.started) return DWGSIM_HIP_OK;
    j->me.started = true;
    auto &c = j->cfg;
    std::vector<const char *> nm; for (auto &s : c.tab_names) nm.push_back(s.c_str());
    for (int d = 0; d < c.ND; ++d) {
        dwgsim_hip_ctx_t *x = c.ctx[(size_t)d].get();
        if (!c.regions_path.empty()) {      // dwgsim.c:499-506
            uint64_t tl = 0;
            if (dwgsim_hip_set_regions(x, c.regions_path.c_str(), nm.data(), c.tab_lens.data(), (int)nm.size(), &tl) < 0) { job_fail(j, dwgsim_hip_last_error(x)); return DWGSIM_HIP_ERR_ARG; }
            c.tot_len = tl;
        }
        if (c.mutin_type >= 0 &&            // dwgsim.c:494-497
            dwgsim_hip_set_mutation_input(x, c.mutin_type, c.mutin_path.c_str(), nm.data(), c.tab_lens.data(), (int)nm.size()) < 0) { job_fail(j, dwgsim_hip_last_error(x)); return DWGSIM_HIP_ERR_ARG; }
        if (c.gzip && c.want_reads && c.has_sink() && dwgsim_hip_set_gzip(x, 1) < 0) { job_fail(j, dwgsim_hip_last_error(x)); return DWGSIM_HIP_ERR_DEVICE; }
        if (c.tvcf_fn) { const int rc = dwgsim_hip_set_truth_depth(x, 1); if (rc < 0) { job_fail(j, dwgsim_hip_last_error(x)); return rc; } }
        if (c.truth_sam && c.want_reads) { int rc = dwgsim_hip_set_truth_sam(x, 1); if (rc >= 0 && c.truth_md) rc = dwgsim_hip_set_truth_md(x, 1); if (rc < 0) { job_fail(j, dwgsim_hip_last_error(x)); return rc; } }      // (-M 2: no reads, no SAM)
    }
    for (int d = 0; d < c.ND; ++d) j->me.workers.emplace_back([j, d]() { Worker w{j, d, j->cfg.ctx[(size_t)d].get()}; w.run(); });
    if (c.want_reads && c.has_sink())      // reads_at: a thread per device and stream; reads: one per stream
        for (int dev = c.sink.reads_at ? 0 : -1; dev < (c.sink.reads_at ? c.ND : 0); ++dev)
            for (int s = 0; s < (c.truth_sam ? JOB_STREAMS : 3); ++s) j->me.deliverers.emplace_back([j, dev, s]() { deliver_loop(j, dev, s); });      // (the truth SAM: a thread of its own, like a FASTQ stream)
    return DWGSIM_HIP_OK;
}

// The contig loop's scheduling for one contig (dwgsim.c:535-625): its length for fragment placement and its number of pairs -- or the reason it is
// passed over, with the reference's message.  -> pairs (>= 0), or a DWGSIM_HIP_SKIP_ value
int64_t schedule_contig(dwgsim_hip_job *j, const char *name, uint32_t ci, const uint8_t *ascii, int64_t l, int64_t *l_eff)
{
    const dwgsim_hip_params_t &o = j->cfg.prm; auto &me = j->me;
    *l_eff = l;
    if (!j->cfg.want_reads) return 0;
    const bool last_takes_rest = me.n_ref == 0 && o.C < 0;     // dwgsim.c:535-537
    if (!j->cfg.regions_path.empty() && !last_takes_rest) {
        int64_t num_n = 0, m = 0;
        *l_eff = dwgsim_hip_contig_region_length(j->cfg.ctx[0].get(), ci, ascii, l, &num_n, &m);
        if (*l_eff == DWGSIM_HIP_SKIP_NO_REGION) { say(j, "[dwgsim_core] #0 skip sequence '%s' as it is not in the targeted region\n", name); return *l_eff; }
        if (*l_eff == DWGSIM_HIP_SKIP_NON_ACGT) { say(j, "[dwgsim_core] #1 skip sequence '%s' as %d out of %d bases are non-ACGT\n", name, (int)num_n, (int)m); return *l_eff; }      // dwgsim.c:575
    }
    const int64_t n_pairs = dwgsim_hip_pairs_for_contig(&o, *l_eff, j->cfg.tot_len, me.n_ref == 0, me.n_sim);
    if (n_pairs < 0) {
        if (!me.prev_skip) say(j, "\n");
        me.prev_skip = 1;
        // (the reference prints its `l`, which is the region length once -x is in force: dwgsim.c:552, :601, :615)
        if (n_pairs == DWGSIM_HIP_SKIP_AMPLICON) say(j, "[dwgsim_core] #2 skip sequence '%s' as it is shorter than the read length %d < %d!\n", name, (int)*l_eff, o.length[0] > o.length[1] ? o.length[0] : o.length[1]);
        else if (n_pairs == DWGSIM_HIP_SKIP_SHORT_INSERT) say(j, "[dwgsim_core] #3 skip sequence '%s' as it is shorter than %f!\n", name, o.dist + 3 * o.std_dev);
        else if (n_pairs == DWGSIM_HIP_SKIP_SHORT_READ) say(j, "[dwgsim_core] #4 skip sequence '%s' as it is shorter than %d!\n", name, (*l_eff < o.length[0]) ? o.length[0] : o.length[1]);
        else say(j, "[dwgsim_core] #5 skip sequence '%s' as not enough pairs found\n", name);
        return n_pairs;
    }
    me.prev_skip = 0;
    me.n_sim += n_pairs;
    return n_pairs;
}

// a staging slot for a new group to be filled in: waits until one of the two is free.  -> the slot, or -1: the job has failed
int take_stage_slot(dwgsim_hip_job *j)
{
    std::unique_lock<std::mutex> lk(j->m);
    int slot = -1;
    j->cv.wait(lk, [&]() {
        retire_loop_step(j);
        for (int s = 0; s < dwgsim_hip_job::Caller::N_STAGE && slot < 0; ++s) if (!j->sh.stage_busy[s]) slot = s;
        return j->failed.load() || slot >= 0;
    });
    if (j->failed.load()) return -1;
    j->sh.stage_busy[slot] = true;
    return slot;
}

} // namespace

extern "C" {

dwgsim_hip_job_t *dwgsim_hip_job_create(const dwgsim_hip_params_t *p, const int *devices, int n_devices, const dwgsim_hip_job_sink_t *sink,
                                        const dwgsim_hip_job_options_t *opt, int *err)
{
    auto bad = [&](int e) { if (err) *err = e; return (dwgsim_hip_job_t *)nullptr; };
    if (!p) return bad(DWGSIM_HIP_ERR_ARG);
    std::vector<int> devs;
    if (n_devices <= 0 || !devices) { const int n = dwgsim_hip_device_count(); for (int d = 0; d < n; ++d) devs.push_back(d); }      // every device the process sees
    else devs.assign(devices, devices + n_devices);
    if (devs.empty()) { fprintf(stderr, "dwgsim-hip: no usable HIP device; the hot path has no CPU fallback\n"); return bad(DWGSIM_HIP_ERR_DEVICE); }
    int solo_r = -1, solo_w = 0;
    if (const char *e = getenv("DWGSIM_HIP_SOLO")) {      // "r/W": measurement only (struct dwgsim_hip_job)
        if (sscanf(e, "%d/%d", &solo_r, &solo_w) != 2 || solo_w < 1 || solo_r < 0 || solo_r >= solo_w) { fprintf(stderr, "dwgsim-hip: DWGSIM_HIP_SOLO wants r/W with 0 <= r < W\n"); return bad(DWGSIM_HIP_ERR_ARG); }
        devs.resize(1);
    }
    std::unique_ptr<dwgsim_hip_job> j(new dwgsim_hip_job());
    auto &c = j->cfg;
    c.tracing = getenv("DWGSIM_HIP_TRACE") != nullptr; c.t0 = mono_s();
    c.prm = *p;
    if (p->read_prefix) { c.prefix = p->read_prefix; c.prm.read_prefix = c.prefix.c_str(); }
    if (p->flow_order) { c.flow = p->flow_order; c.prm.flow_order = c.flow.c_str(); }
    memset(&c.sink, 0, sizeof c.sink); if (sink) c.sink = *sink;
    memset(&c.opt, 0, sizeof c.opt); if (opt) c.opt = *opt; else c.opt.gzip = 1;
    c.gzip = c.opt.gzip != 0;
    if (c.opt.batch_pairs) c.batch_pairs = c.opt.batch_pairs;
    if (c.opt.group_bp) c.group_bp = c.opt.group_bp;
    if (c.opt.min_share) c.min_share = c.opt.min_share;
    c.want_mut = p->output_type != 1; c.want_reads = p->output_type != 2;
    c.devices = devs; c.ND = (int)devs.size();
    c.VD = solo_r >= 0 ? solo_w : c.ND; c.solo_rank = solo_r;
    c.ctx.resize((size_t)c.ND);
    {   // one context per device, made side by side (a context costs about 0.1 s of runtime set-up, code objects and buffers)
        std::vector<int> errs((size_t)c.ND, 0);
        std::vector<std::thread> th;
        dwgsim_hip_params_t rest = c.prm;
        const bool calibrates = c.prm.data_type == 2 && c.prm.use_base_error;      // -B (dwgsim_opt.c:415-457): once, on the first device; the others take its result
        if (calibrates) {
            c.ctx[0].reset(dwgsim_hip_create(&c.prm, devs[0], &errs[0]));
            if (c.ctx[0] && dwgsim_hip_get_params(c.ctx[0].get(), &rest) == DWGSIM_HIP_OK) { rest.use_base_error = 0; rest.read_prefix = c.prm.read_prefix; rest.flow_order = c.prm.flow_order; }
        }
        for (int d = 1; d < c.ND; ++d) th.emplace_back([&, d]() { c.ctx[(size_t)d].reset(dwgsim_hip_create(&rest, devs[(size_t)d], &errs[(size_t)d])); });
        if (!calibrates) c.ctx[0].reset(dwgsim_hip_create(&c.prm, devs[0], &errs[0]));
        for (auto &t : th) t.join();
        for (int d = 0; d < c.ND; ++d)
            if (!c.ctx[(size_t)d]) {
                const int e = errs[(size_t)d];
                fprintf(stderr, "dwgsim-hip: cannot create a GPU context on device %d (error %d)\n", devs[(size_t)d], e);
                return bad(e ? e : DWGSIM_HIP_ERR_DEVICE);
            }
    }
    j->sh.next_group.assign((size_t)c.ND, 0);
    j->sh.bufs.resize((size_t)c.ND); j->sh.free_bufs.resize((size_t)c.ND);
    trace(j.get(), "contexts made");
    if (err) *err = DWGSIM_HIP_OK;
    return j.release();
}

int dwgsim_hip_job_set_contig_table(dwgsim_hip_job_t *j, const char *const *names, const int64_t *lens, int n)
{
    if (!j || n < 0 || (n && (!names || !lens)) || j->me.started) return arg_error(j, DWGSIM_HIP_ERR_ARG, "job: the contig table must be set once, before the first contig");
    auto &c = j->cfg;
    c.tab_names.clear(); c.tab_lens.clear(); c.tot_len = 0;
    for (int i = 0; i < n; ++i) { c.tab_names.push_back(names[i]); c.tab_lens.push_back(lens[i]); c.tot_len += (uint64_t)lens[i]; }
    j->me.n_ref = n; c.have_table = true;
    // room for the largest group (consecutive contigs up to group_bp, or one longer contig alone), so that each staging buffer is page-locked once
    int64_t longest = 0; for (int i = 0; i < n; ++i) longest = std::max<int64_t>(longest, (lens[i] + 4095) / 4096 * 4096);
    c.stage_want = (size_t)std::max<int64_t>(longest, (int64_t)std::min<uint64_t>(c.group_bp, (uint64_t)c.tot_len + 4096 * (uint64_t)n)) + 8192;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_job_set_regions(dwgsim_hip_job_t *j, const char *path)
{
    if (!j || !path || j->me.started) return arg_error(j, DWGSIM_HIP_ERR_ARG, "job: regions must be set before the first contig");
    j->cfg.regions_path = path;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_job_set_mutation_input(dwgsim_hip_job_t *j, int type, const char *path)
{
    if (!j || !path || type < 0 || type > 2 || j->me.started) return arg_error(j, DWGSIM_HIP_ERR_ARG, "job: the mutation input must be set before the first contig");
    j->cfg.mutin_type = type; j->cfg.mutin_path = path;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_job_set_chain_sink(dwgsim_hip_job_t *j, dwgsim_hip_job_chain_fn fn, void *user)
{
    if (!j) return DWGSIM_HIP_ERR_ARG;
    if (j->me.started) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: the chain sink must be set before the first contig");
    j->cfg.chain_fn = fn; j->cfg.chain_user = user;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_job_set_haplotype_sink(dwgsim_hip_job_t *j, dwgsim_hip_job_haplotype_fn fn, void *user, int width)
{
    if (!j || width < 0) return arg_error(j, DWGSIM_HIP_ERR_ARG, "job: the haplotype line width must not be negative");
    if (j->me.started) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: the haplotype sink must be set before the first contig");
    j->cfg.hap_fn = fn; j->cfg.hap_user = user; j->cfg.hap_width = width;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_job_set_truth_vcf_sink(dwgsim_hip_job_t *j, dwgsim_hip_job_truth_vcf_fn fn, void *user)
{
    if (!j) return DWGSIM_HIP_ERR_ARG;
    if (j->me.started) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: the truth VCF sink must be set before prepare / the first contig");
    if (fn && j->cfg.prm.data_type != 0) return arg_error(j, DWGSIM_HIP_ERR_UNSUP, "dwgsim-hip: the truth VCF is made for Illumina reads only (-c 0)\n");
    j->cfg.tvcf_fn = fn; j->cfg.tvcf_user = user;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_job_set_truth_sam(dwgsim_hip_job_t *j, int on)
{
    if (!j) return DWGSIM_HIP_ERR_ARG;
    if (j->me.started) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: the truth SAM must be switched on before prepare / the first contig");
    if (on && j->cfg.prm.data_type != 0) return arg_error(j, DWGSIM_HIP_ERR_UNSUP, "dwgsim-hip: the truth SAM is made for Illumina reads only (-c 0)\n");
    j->cfg.truth_sam = on != 0;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_job_set_truth_md(dwgsim_hip_job_t *j, int on)
{
    if (!j) return DWGSIM_HIP_ERR_ARG;
    if (j->me.started) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: the NM / MD tags of the truth SAM must be switched on before prepare / the first contig");
    if (on && j->cfg.prm.data_type != 0) return arg_error(j, DWGSIM_HIP_ERR_UNSUP, "dwgsim-hip: the truth SAM and its NM / MD tags are made for Illumina reads only (-c 0)\n");
    j->cfg.truth_md = on != 0;
    return DWGSIM_HIP_OK;
}

// test / analysis hooks: dwgsim_hip_debug_option on every context of the job (before the first contig), dwgsim_hip_debug_get summed over them (after finish)
int dwgsim_hip_job_debug_option(dwgsim_hip_job_t *j, const char *key, int64_t value)
{
    if (!j || !key) return DWGSIM_HIP_ERR_ARG;
    if (j->me.started) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: debug options must be set before prepare / the first contig");
    for (auto &x : j->cfg.ctx) { const int rc = dwgsim_hip_debug_option(x.get(), key, value); if (rc < 0) return arg_error(j, rc, dwgsim_hip_last_error(x.get())); }
    return DWGSIM_HIP_OK;
}
int dwgsim_hip_job_debug_get(dwgsim_hip_job_t *j, const char *key, int64_t *value)
{
    if (!j || !key || !value) return DWGSIM_HIP_ERR_ARG;
    if (j->me.started && !j->me.finished) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: debug values are read before the first contig or after finish");
    *value = 0;
    for (auto &x : j->cfg.ctx) { int64_t v = 0; const int rc = dwgsim_hip_debug_get(x.get(), key, &v); if (rc < 0) return arg_error(j, rc, dwgsim_hip_last_error(x.get())); *value += v; }
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_job_prepare(dwgsim_hip_job_t *j, uint64_t *total_len)
{
    if (!j || !j->cfg.have_table) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: set the contig table first");
    const int rc = start_threads(j);
    if (total_len) *total_len = j->cfg.tot_len;
    return rc;
}

// The contig loop's body (dwgsim.c:519-625) in two halves, so that the caller can produce the sequence in place -- and with as many threads as it
// likes: begin reserves the contig's bytes in the page-locked staging of the group being filled (group layout), commit schedules it.
uint8_t *dwgsim_hip_job_begin_contig(dwgsim_hip_job_t *j, const char *name, int64_t l, int64_t *status)
{
    auto out = [&](int64_t st) { if (status) *status = st; return (uint8_t *)nullptr; };
    if (!j || !name || l < 0 || l > INT32_MAX) return out(arg_error(j, DWGSIM_HIP_ERR_ARG, "job: bad contig arguments"));
    if (!j->cfg.have_table) return out(arg_error(j, DWGSIM_HIP_ERR_STATE, "job: set the contig table first (the reference reads it before the first contig: dwgsim.c:465-478)"));
    auto &me = j->me; const auto &c = j->cfg;
    if (me.finished) return out(arg_error(j, DWGSIM_HIP_ERR_STATE, "job: already finished"));
    if (me.open.open) return out(arg_error(j, DWGSIM_HIP_ERR_STATE, "job: the previous contig was neither committed nor cancelled"));
    if (start_threads(j) < 0) return out(DWGSIM_HIP_ERR_FAILED);
    if (j->failed.load()) return out(DWGSIM_HIP_ERR_FAILED);
    // into the group being filled; a contig that would take it past the group size closes it first
    const int64_t aligned_len = (l + 4095) / 4096 * 4096;
    if (me.pending && me.pending_bytes + (size_t)aligned_len > (size_t)c.group_bp) { if (dispatch_pending(j) < 0) return out(DWGSIM_HIP_ERR_FAILED); }
    if (!me.pending) {
        auto g = std::make_shared<GroupJob>();
        if ((g->stage_slot = take_stage_slot(j)) < 0) return out(DWGSIM_HIP_ERR_FAILED);
        me.pending = g; me.pending_bytes = 0;
    }
    GroupJob &g = *me.pending;
    // the contig's place in the group layout (dwgsim_hip_group_layout): the next multiple of 4096
    std::vector<int64_t> lens = g.lens; lens.push_back(l);
    std::vector<int64_t> starts(lens.size());
    const int64_t total = dwgsim_hip_group_layout(lens.data(), (int)lens.size(), starts.data());
    const int s = g.stage_slot;
    if (!me.stage[s].p || (size_t)total > me.stage[s].cap) {      // grow, keeping what the group already holds (an empty record that opens a group on a fresh slot still needs somewhere to point)
        // (the contig table says how large a group can get: exactly that much; a table that understated the lengths -- a stale .fai -- grows by a quarter)
        const size_t want = (size_t)total <= c.stage_want ? c.stage_want : std::max<size_t>((size_t)total + (size_t)total / 4, (size_t)std::min<uint64_t>(c.group_bp, 256u << 20) + 8192);
        trace(j, "staging %d: page-locking %.0f MB", s, want / 1e6);
        const bool got = me.stage[s].grow(want, me.pending_bytes);
        trace(j, "staging %d: done", s);
        if (!got) { job_fail(j, "dwgsim-hip: cannot allocate page-locked host memory for the sequence"); return out(DWGSIM_HIP_ERR_NOMEM); }
    }
    uint8_t *base = me.stage_at(s);
    const int64_t st = starts.back();
    if ((size_t)st > me.pending_bytes) memset(base + me.pending_bytes, 0, (size_t)st - me.pending_bytes);      // zero bytes between the contigs
    if ((size_t)total > (size_t)(st + l)) memset(base + st + l, 0, (size_t)total - (size_t)(st + l));
    me.open.open = true; me.open.name = name; me.open.l = l; me.open.st = st; me.open.total = total; me.open.ci = me.next_index;
    if (status) *status = DWGSIM_HIP_OK;
    return base + st;
}

int dwgsim_hip_job_cancel_contig(dwgsim_hip_job_t *j)
{
    if (!j || !j->me.open.open) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: no contig is open");
    j->me.open.open = false;      // (the reserved bytes are simply handed out again)
    return DWGSIM_HIP_OK;
}

int64_t dwgsim_hip_job_commit_contig(dwgsim_hip_job_t *j)
{
    if (!j || !j->me.open.open) return arg_error(j, DWGSIM_HIP_ERR_STATE, "job: no contig is open");
    auto &me = j->me;
    me.open.open = false;
    if (j->failed.load()) return DWGSIM_HIP_ERR_FAILED;
    GroupJob &g = *me.pending;
    const uint32_t ci = me.next_index++;
    --me.n_ref;
    int64_t l_eff = 0;
    const int64_t n_pairs = schedule_contig(j, me.open.name.c_str(), ci, me.stage_at(g.stage_slot) + me.open.st, me.open.l, &l_eff);
    if (n_pairs < 0) return n_pairs;      // passed over: its bytes are handed out again
    me.pending_bytes = (size_t)me.open.total;
    g.names.push_back(me.open.name); g.lens.push_back(me.open.l); g.l_eff.push_back(l_eff); g.n_pairs.push_back(n_pairs); g.cindex.push_back(ci);      // (where the sequences stand is resolved at dispatch: the staging may still move)
    if (me.pending_bytes >= (size_t)j->cfg.group_bp && dispatch_pending(j) < 0) return DWGSIM_HIP_ERR_FAILED;
    return n_pairs;
}

int64_t dwgsim_hip_job_add_contig(dwgsim_hip_job_t *j, const char *name, const uint8_t *ascii, int64_t l)
{
    if (j && !ascii && l > 0) return arg_error(j, DWGSIM_HIP_ERR_ARG, "job: bad contig arguments");
    int64_t st = 0;
    uint8_t *dst = dwgsim_hip_job_begin_contig(j, name, l, &st);
    if (st < 0 || !dst) return st < 0 ? st : arg_error(j, DWGSIM_HIP_ERR_STATE, "job: begin_contig returned no place for the sequence");      // (the status decides, not the pointer)
    if (l > 0) memcpy(dst, ascii, (size_t)l);
    return dwgsim_hip_job_commit_contig(j);
}

int dwgsim_hip_job_finish(dwgsim_hip_job_t *j)
{
    if (!j) return DWGSIM_HIP_ERR_ARG;
    if (j->me.finished) return j->failed.load() ? DWGSIM_HIP_ERR_FAILED : DWGSIM_HIP_OK;
    j->me.finished = true;
    if (!j->failed.load()) (void)dispatch_pending(j);
    { std::lock_guard<std::mutex> lk(j->m); j->sh.no_more = true; j->cv.notify_all(); }
    for (auto &t : j->me.workers) t.join();
    for (auto &t : j->me.deliverers) t.join();
    { std::lock_guard<std::mutex> lk(j->m); if (!j->failed.load()) retire_loop_step(j); }
    return j->failed.load() ? DWGSIM_HIP_ERR_FAILED : DWGSIM_HIP_OK;
}

const char *dwgsim_hip_job_last_error(const dwgsim_hip_job_t *j) { return j ? j->sh.err.c_str() : "no job"; }

void dwgsim_hip_job_destroy(dwgsim_hip_job_t *j)
{
    if (!j) return;
    if (!j->me.finished) { job_fail(j, "job destroyed before it was finished"); (void)dwgsim_hip_job_finish(j); }
    delete j;
}

} // extern "C"
