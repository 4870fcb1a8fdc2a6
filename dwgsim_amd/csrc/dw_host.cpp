// dw_host.cpp -- C-ABI (include/dwgsim_hip.h) over the HIP kernels of dw_walk.hip / dw_simulate.hip.
//
// Host responsibilities, mirroring what dwgsim_core() does around its two hot loops:
//   * option defaults / checks / error-ramp tables      (dwgsim_opt.c:40-80, :307-371, :459-460)
//   * contig scheduling arithmetic                       (dwgsim.c:535-537, :582-590, :595-618)
//   * device residency of contigs and mutated haplotypes (replaces seq_t / mutseq_t, mut.h:12-47)
//   * mutations.txt / .vcf text from the sparse list of mutated cells (mut.c:781-893)
// There is no CPU implementation of the hot path here: without a HIP device create() fails.
//
// Contigs are resident in GROUPS: the contigs of one dwgsim_hip_add_contigs call share one coordinate space (contig k at a multiple of
// GROUP_ALIGN cells, unmutated N between them), one chain of walk kernels mutates all of them, and one k_simulate launch can cover read-index
// ranges of several of them -- so a job of thousands of small contigs (the reference's contig loop, dwgsim.c:519-625, has no fixed cost per
// contig) pays the walk chain, the launches and the host synchronisations once per group instead of once per contig.  A group of one contig
// is the plain case.
// Every device resource has an owner (dw_mem.hpp: DevMem, HostMem, DevEvent, DevStream), so a context is created in named steps (open_streams ..
// upload_rand_name) that may fail anywhere, and destroyed by waiting for its streams and deleting it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <ctype.h>
#include <stdarg.h>
#include <stdint.h>
#include <sys/mman.h>
#include <mutex>
#include <thread>
#include <string>
#include <vector>
#include <algorithm>
#include <array>
#include <stddef.h>
#include <type_traits>
#include "../../include/dwgsim_hip.h"
#include "dw_kernels.hpp"
#include "dw_launch.hpp"
#include "dw_mutin.hpp"
#include "dw_mem.hpp"

using namespace dw;

namespace {

struct HostIns { std::vector<int32_t> pos; std::vector<uint32_t> len, off; std::vector<uint8_t> bases; };

struct Member {                      // one contig of a group
    std::string name;
    int64_t l = 0, l_place = 0;      // length; fragment-placement length (region length with -x)
    uint32_t contig_index = 0;       // ordinal in the FASTA (RNG key)
    int32_t start = 0;               // first cell in the group's coordinate space
    int32_t reg_off = 0, n_reg = 0;  // -x: [starts | ends] of this contig in the group's region pool
    uint32_t name_off = 0; int32_t name_fixed_len = 0;      // "@[prefix_]name" in the group's name pool
    ResolvedContig rc;               // -m / -b / -v: the file's entries for this contig, resolved when the contig was added
};

// What a dropped group leaves for the next one (dwgsim_hip_ctx::pool): its device memory, the events and page-locked counters of its walk, and the
// host sources of its uploads.  The buffers of cells are sized for d_ref.cap() padded cells.
struct GroupMem {
    DevMem d_ref, d_cells[2], d_view[2];      // reference codes, byte cells, 4-bit read views
    DevMem d_ins_pos[2], d_ins_len[2], d_ins_off[2], d_ins_bases[2];      // insertion tables (int32 / uint32 entries; inserted bases + 16 bytes)
    DevMem d_names, d_reg, d_seg;            // name pool, region pool, segment table (start[n + 1] | len[n] | cindex[n])
    std::vector<uint8_t> h_names; std::vector<int32_t> h_reg, h_seg;      // their host sources (alive while asynchronous copies may read them)
    DevMem d_summ[2], d_summ2[2];            // haplotype summaries (uint16, per 64 and per 1024 cells) for count_random: kept in step with the read views
    // the walk as sparse work (dw_walk.hip k_mark_dirty / k_dirty_chunks): the view and the summaries of the UNMUTATED group, made once at upload, and
    // the bitmap (uint32) of 64-cell chunks the last walk may have written
    DevMem d_refview, d_refsumm, d_refsumm2, d_dirty;
    DevEvent ev_walk, ev_walk0;      // end / start of the walk chain on the walk stream
    DevMem d_hap_text[2], d_hap_rec, d_hap_pool;      // dwgsim_hip_haplotype_fasta (empty until it is called): each haplotype's FASTA text; the records and header lines of the text made last
    DevMem d_hap_chain[2];           // dwgsim_hip_haplotype_chain (empty until it is called): each haplotype's block ends (ChainEnt), sized from the count the device made
    DevMem d_depth_pos, d_depth_cnt;      // dwgsim_hip_set_truth_depth (empty until a batch runs with it): the group's listed cells (int32, ascending) and two u64 counters per cell (dw_kernels.hpp DepthArgs)
    HostMem h_wc;                    // page-locked mirror (a WalkCounters) of the walk's counters (the context's d_wcounters) at the end of THIS group's walk: several groups' walks can be in flight
};

// The walk's counter block: 16 u64 words, on the device (dwgsim_hip_ctx::d_wcounters) and mirrored per group (GroupMem::h_wc).  The kernels are handed pointers to
// single words of it, so the layout is the host's alone.  The random walk clears and reads back n_cand .. n_cand_true, the file-driven walk mut_debug (WC_*).
struct WalkCounters {
    uint64_t unused0[7];
    uint64_t n_cand;                                 // candidate sites in the list (0 when a slot overflowed)
    uint32_t max_del;                                // longest deletion run (k_events -> k_resolve)
    struct { uint32_t entries, bases; } ins[2];      // insertion-table entries and inserted bases per haplotype (the tot4 of k_resolve / k_apply)
    uint32_t unused1;
    uint32_t slot_over;                              // a block of the site scan outgrew its slot: nothing behind it ran
    uint32_t n_cand_true;                            // ... and the candidates there really are
    uint64_t mut_debug[2];                           // the file-driven walk: mut_debug verdict before / after the justification (all ones: none)
    uint64_t n_listed;                               // mutated cells (fetch_mutated_list)
    uint64_t unused2;
};
static_assert(std::is_standard_layout<WalkCounters>::value && sizeof(WalkCounters) == 16 * 8, "the walk's counter block is 16 u64 words");
static_assert(offsetof(WalkCounters, n_cand) == 7 * 8 && offsetof(WalkCounters, max_del) == 8 * 8 && offsetof(WalkCounters, ins) == 8 * 8 + 4 && offsetof(WalkCounters, slot_over) == 8 * 8 + 6 * 4 &&
              offsetof(WalkCounters, n_cand_true) == 8 * 8 + 7 * 4 && offsetof(WalkCounters, mut_debug) == 12 * 8 && offsetof(WalkCounters, n_listed) == 14 * 8, "every counter at the word the kernels were given before the block had a type");
struct WcSpan { size_t off, bytes; };      // the fields `first` through `last`, as bytes of the block
#define WC_SPAN(first, last) WcSpan{offsetof(WalkCounters, first), offsetof(WalkCounters, last) + sizeof(WalkCounters::last) - offsetof(WalkCounters, first)}
constexpr WcSpan WC_RANDOM = WC_SPAN(n_cand, n_cand_true), WC_FILE = WC_SPAN(mut_debug, mut_debug), WC_LISTED = WC_SPAN(n_listed, n_listed);

struct Group {
    bool alive = false, mutated = false, walk_pending = false;
    int first_handle = -1;
    std::vector<Member> m;
    int64_t total = 0;               // cells of the coordinate space (a multiple of 16; allocations add CELL_PAD = 64: a whole 64-cell chunk past the last cell stays inside)
    GroupMem mem;
    uint32_t n_ins[2] = {0, 0}, n_ins_bases[2] = {0, 0};
    int fixed_max = 0;               // longest "[prefix_]name"
    uint32_t n_cand = 0;
    bool dirty_any = false, dirty_all = false;      // mem.d_dirty: any chunk written -- or "everything" after a walk that kept no bitmap (dirty_all)
    // a walk that was enqueued and not yet waited for
    int walk_attempt = 0; uint32_t walk_cap = 0; size_t walk_cap_bases = 0; bool walk_reset = false;
    uint32_t n_patch = 0, n_patch_ev = 0;       // file-driven mutations: patched cells / indel events
    // the mutated cells of the finished walk, fetched once for mutations_text
    bool list_valid = false; std::vector<int32_t> pos; std::vector<uint32_t> cells; HostIns ins[2];
    // the true read depth: the listed cells of the finished walk as mem.d_depth_pos holds them (host copy: a contig's slice), the counters zeroed behind them (depth_prepare)
    bool depth_valid = false; std::vector<int32_t> depth_pos;
    // the FASTA text of each finished haplotype (mem.d_hap_text), made on request: its width and size, and per contig where the record lies and its bases
    struct HapText { bool valid = false; int width = 0; uint64_t bytes = 0; std::vector<uint64_t> off, len; std::vector<int64_t> bases; } hap_text[2];
    // the ungapped blocks of each finished haplotype against the reference (mem.d_hap_chain, paired by the host), made on request: contig k's are blocks[first[k] .. first[k + 1])
    struct HapChain { bool valid = false; std::vector<uint64_t> first; std::vector<int64_t> ref_start; std::vector<dwgsim_hip_chain_block_t> blocks; } hap_chain[2];
};

struct HandleRef { int group = -1, k = 0; };

struct Counters {                   // a device counter block (its layout: dw_kernels.hpp) and its page-locked mirror
    DevMem d; HostMem h;
    uint64_t *dev() const { return d.get<uint64_t>(); }
    uint64_t *host() const { return h.get<uint64_t>(); }
};

struct Slot {                       // one of the two batches a context can have in flight
    Counters counters;
    DevEvent ev_k0, ev_k1, ev_end, ev_done, ev_fetched;
    DevEvent ev_t0, ev_t1;          // around the truth step (made by dwgsim_hip_set_truth_sam: a context that never switches it on has none)
    bool pending = false, empty = true, fetch_in_flight = false;
    bool truth_timed = false;       // the batch in flight recorded ev_t0 / ev_t1 (it ran the truth step, or its depth counters alone)
    int group = -1;                 // the group the batch in flight reads
    uint64_t n_pairs = 0, out_bytes[N_STREAMS] = {0, 0, 0, 0}, gz_bytes[N_STREAMS] = {0, 0, 0, 0};
    DevMem gz_out[N_STREAMS], gz_status, segs;        // GPU gzip: the members of each stream, look-back words; the range table of the launch
    HostMem h_segs;                           // ... and its page-locked source
    std::vector<dwgsim_hip_range_t> ranges;      // what the batch in flight covers (it is enqueued again, with larger read buffers, when an Ion Torrent read outgrew them)
    DevMem d_rerun_chain;                        // [2]: the chain words such a second run starts from
    int cap_mult = 1;                            // the context's flow_cap_mult this batch was enqueued with
};

} // namespace

// Every member that owns something of the device (DevMem, HostMem, DevEvent, DevStream, and the groups, pool and slots made of them) gives it back in its destructor,
// in the reverse of the order below.  Any order is safe: dwgsim_hip_destroy synchronises every stream that exists before it deletes the context, so nothing in
// flight reads a buffer, waits for an event or runs on a stream when the first member goes, and no member's destructor looks at another member.
struct dwgsim_hip_ctx {
    dwgsim_hip_params_t prm;
    std::string read_prefix;
    // What dwgsim_hip_create's upload steps make once per context (upload_flow_order, upload_error_tables per read end, upload_rand_name); fill_sim_args hands them to the kernels
    struct Tables {
        std::vector<uint8_t> flow;            // Ion Torrent flow order as base codes
        DevMem d_flow;                        // ... its 64 bytes on the device, and behind them the log2 table of the gap draws
        double e_by[2] = {0, 0};
        DevMem d_thr[2];                         // u64
        DevMem d_thr32[2]; int e_full = 0;       // u32
        DevMem d_qbase[2]; int32_t qb_words = 1;      // u32
        DevMem d_rand_fixed; int32_t rand_fixed_len = 0;
    } tab;
    // The test / analysis knobs dwgsim_hip_debug_option sets and the values dwgsim_hip_debug_get reads back (the keys in quotes; what each means: at those two functions)
    struct Debug {
        int site_slots = -1; int64_t site_slot_cap = -1;      // "site_slots": -1 choose, 0 the look-back form, 1 the slot form; "site_slot_cap": a slot size to start from (tests: the overflow re-run)
        bool seq_justify = false, dense_view = false;      // "justify_seq", "dense_view": the cross-check forms of the walk (one thread justifies a whole group; the views are made from every cell)
        int flow_cap_forced = 0;               // "flow_cap" (tests): the capacity a job starts from, instead of flow_read_capacity()
        int ion_lds = -1;                      // "ion_lds" (tests): where the Ion Torrent read buffers live (fill_sim_args)
        int flow_slots = 0;                    // "flow_slots": scratch slots per XCD forced by the tests (0: as many as an XCD can hold blocks)
        int64_t truth_cap = -1, truth_reruns = 0;      // "truth_cap": the capacity (bytes) a batch's truth SAM is planned with at first (-1: the product's own); "truth_reruns": second runs that found the room (dwgsim_hip_set_truth_md)
        int64_t walk_cap = -1, place_cap = -1; bool phases = false;      // "walk_cap", "place_cap": capacities to start too small from (-1: the product's own); "phases": print the phase split of the -DDW_PHASE_TIMING build
        int writer = -1, force_threads = 0, split = -1, qrows = 1;      // "writer", "sim_threads", "split", "qrows": the k_simulate form forced (choose_sim_form)
        uint64_t place_open = 0; double walk_us = 0, count_us = 0;      // "place_open", "walk_us", "count_us": read back
        int64_t sim_form = 0;                  // dwgsim_hip_debug_get("sim_form"): the k_simulate form of the last launch
        int64_t walk_form = 0;                 // dwgsim_hip_debug_get("walk_form"): what the last walk enqueued was made of
        double hap_len_us = 0, hap_write_us = 0, hap_copy_us = 0, truth_us = 0, truth_copy_us = 0; bool hap_yardstick = false; double chain_count_us = 0, chain_write_us = 0; int64_t chain_blocks = 0;      // "chain_count_us" / "chain_write_us" / "chain_blocks"; "hap_len_us" / "hap_write_us" / "hap_copy_us", "hap_yardstick" (dwgsim_hip_debug_get / _option)
    } dbg;
    int device = 0;
    DevStream stream;            // simulate: kernels of the batches
    DevStream copy_stream;       // device -> host copies of finished text
    DevStream walk_stream;       // uploads, the mutation walk, the mutated-cell list: a group can be prepared while another one is being simulated
    DevStream count_stream;      // count_random (k_place ..): behind the walk of ITS group only (an event), not behind the walks of groups issued later --
                                 // on the walk stream the count of step k+1 waited for the walks of steps k+2, k+3 (round 6: profiles/r06_solo_rank_entry.txt)
    std::string err;
    std::vector<Group> groups;
    std::vector<GroupMem> pool;              // the device memory, events and page-locked mirrors of dropped groups, handed to the next add_contigs whose cells fit: a
                                             // job of many groups pays its hipMalloc / hipFree (each a device-wide synchronisation) once, not at every group end
    std::vector<HandleRef> handles;          // contig handle -> (group, member); handles are never reused
    // simulate() working set
    DevMem meta, fail_summ, block_rand, status_all, out[DWGSIM_HIP_SLOTS][N_STREAMS], split_state, split_hand, split_agg, split_pre, split_chunk;
    // walk-stream working set (grow-only)
    DevMem w_slots, w_slot_aux;      // the site scan's per-block slots (dw_walk.hip k_site_scan_slots) and their counts / bases
    DevMem scratch_mask, scratch_cnt, scratch_status, w_cand, w_ev, w_flags, w_lo, w_sufmin, w_bound, w_ppos, w_pcells, up_ascii, l_pos, l_cells, place_segs, place_rand, place_list, place_aux;
    HostMem h_up; DevEvent ev_up; bool up_in_flight = false;      // page-locked staging of a group's sequence
    HostMem h_place_segs, h_range_rand;      // page-locked: count_random's range table and its result per range
    std::vector<int32_t> h_ppos; std::vector<uint16_t> h_pcells; std::vector<Event> h_pev;      // file-driven mutations of the group being walked
    MutInput mutin; bool has_mutin = false;                             // -m / -b / -v
    Regions regions; bool has_regions = false;                           // -x
    DevMem flow_scratch, flow_free;
    Counters counters;                       // calibrate / count_random / debug hooks (compute stream)
    DevMem d_wcounters;                      // a WalkCounters (mirrored per group: GroupMem::h_wc)
    Counters pcounters;                      // count_random (walk stream)
    Slot slot[DWGSIM_HIP_SLOTS];             // simulate(): up to three batches in flight (kernels | copy-out issued | copy-out landing: dw_job.cpp)
    DevMem d_chain;                          // [0] random reads emitted before the next batch, [1] the abort rule's carry: handed from batch to batch on the device
    int chain_contig = -1; uint64_t chain_next_ii = 0;      // which (contig, read index) the carry continues
    bool has_carry_override = false; uint64_t carry_override = 0;
    int flow_cap_mult = 1;                 // Ion Torrent: the read capacity is flow_read_capacity() times this; doubled when a read outgrew it (the reference doubles its buffers, dwgsim.c:296-311)
    int n_cu = 0;                          // compute units of the device
    DevEvent ev_cnt0, ev_cnt1;
    bool gzip_on = false; DevMem d_crc_table, d_crc_shift;      // dwgsim_hip_set_gzip (u32; d_crc_shift is uploaded last)
    bool truth_on = false;                 // dwgsim_hip_set_truth_sam: every batch also leaves stream DWGSIM_HIP_STREAM_SAM
    bool truth_md = false;                 // dwgsim_hip_set_truth_md: ... with NM:i: and MD:Z: on every mapped record (nothing while truth_on is off)
    bool depth_on = false;                 // dwgsim_hip_set_truth_depth: every batch adds to its group's counters of the true read depth (with or without the truth SAM)
    DevMem t_nl[2], t_rec[2], t_ends, t_len, t_blk;      // ... its working set (dw_truth.hpp TruthArgs): newline counts and record starts of the source streams, the read ends, the line lengths per end and per block
    HostMem h_stage;                       // pinned staging for fetch
    DevStream hap_stream;                  // dwgsim_hip_haplotype_fetch: copies of its own (made at the first call), not behind the batches' copy-outs
    DevEvent hap_ev[6];                    // dwgsim_hip_haplotype_fasta: the ends of its passes (dbg.hap_*_us)
    DevEvent chain_ev[4];                  // dwgsim_hip_haplotype_chain: around its passes (dbg.chain_*_us), made at its first call
    int hap_cur[2] = {-1, -1};           // ... and the group whose text the last call for that haplotype built or found
    std::string txt, vcf;
};

namespace {

#define HIPC(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { char b_[512]; snprintf(b_, sizeof b_, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #call); (ctx)->err = b_; return DWGSIM_HIP_ERR_DEVICE; } } while (0)

// hipMalloc (DevKind); when the device is out of memory the sets of dropped groups the context keeps for reuse (dwgsim_hip_ctx::pool) are given back and the
// allocation is tried once more -- a job that fitted when groups were freed at drop (rounds 1-4) must not fail with gigabytes idle in the pool
hipError_t dev_malloc(dwgsim_hip_ctx *c, void **p, size_t bytes)
{
    hipError_t e = DevKind::alloc(p, bytes);
    if (e == hipSuccess || c->pool.empty()) return e;
    (void)hipGetLastError();
    hipStreamSynchronize(c->walk_stream.get());
    c->pool.clear();
    return DevKind::alloc(p, bytes);
}

// every device allocation of a context goes through dev_malloc: room for `need` bytes in b, else a new buffer of `want` bytes
hipError_t reserve(dwgsim_hip_ctx *c, DevMem &b, size_t need, size_t want)
{
    return b.reserve(need, want, [c](void **p, size_t n) { return dev_malloc(c, p, n); });
}

// the growth rule of the context's working sets
int ensure(dwgsim_hip_ctx *c, DevMem &b, size_t bytes)
{
    HIPC(c, reserve(c, b, bytes, bytes + bytes / 8 + 4096));
    return 0;
}

// a table of n bytes made once: allocated and copied up (b stays empty when the copy fails, so that the table is made again)
int upload(dwgsim_hip_ctx *c, DevMem &b, const void *src, size_t n)
{
    HIPC(c, reserve(c, b, n, n));
    const hipError_t e = hipMemcpy(b.get(), src, n, hipMemcpyHostToDevice);
    if (e != hipSuccess) b.reset();
    HIPC(c, e);
    return 0;
}

// A host table of a group goes up: room for it and `slack` entries more, then the copy (the vector lives in the GroupMem: the copy may read it after the call)
template <class T> int upload_table(dwgsim_hip_ctx_t *c, DevMem &d, const std::vector<T> &h, size_t slack)
{
    HIPC(c, reserve(c, d, sizeof(T) * h.size(), sizeof(T) * (h.size() + slack)));
    HIPC(c, hipMemcpyAsync(d.get(), h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, c->walk_stream.get()));
    return 0;
}

uint8_t nt4(int ch)      // dwgsim.c:56-73
{
    switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; case '-': return 5; default: return 4; }
}

// Parameters of the lazy quality normals (error budget: dw_simulate.hip quality_try_lazy).  Polar radii with L' = -log2(r) < lmin give
// |nrm| < sqrt(2 ln 2 lmin): lmin is the largest value (<= 2^-4) for which that keeps |nrm * sigma| below 0.45, so the offset is 0 there
// without further work; when sigma is too large for that (lmin would fall below 2^-10) the exact path handles those radii instead.
void lazy_quality_params(double sigma, float *k, float *eps, float *lmin, int32_t *near1_zero)
{
    const double two_ln2 = 2.0 * log(2.0);
    double lm = 0.98 * (0.45 / sigma) * (0.45 / sigma) / two_ln2;
    if (!(lm < 0x1p-4)) lm = 0x1p-4;
    *near1_zero = lm >= 0x1p-10 ? 1 : 0;
    if (lm < 0x1p-10) lm = 0x1p-10;
    *lmin = (float)lm;
    lm = (double)*lmin * (1.0 - 0x1p-20);         // (what the budget may assume after the rounding to float)
    *k = (float)(sqrt(two_ln2) * sigma);
    *eps = (float)(1.5 * sigma * (3.4e-7 / sqrt(lm) + 7.2e-6) + 0x1p-18);       // (+inf for an absurd -Q: every value then takes the exact path)
}

WalkParams walk_params(const dwgsim_hip_ctx *c)
{
    WalkParams w; w.mut_rate = c->prm.mut_rate; w.indel_frac = c->prm.indel_frac; w.indel_extend = c->prm.indel_extend;
    w.indel_min = c->prm.indel_min; w.is_hap = c->prm.is_hap; w.seed = (uint32_t)c->prm.seed;
    w.mut_thr = !(c->prm.mut_rate > 0) ? 0 : c->prm.mut_rate >= 1.0 ? 0x100000000ull : (uint64_t)ceil(c->prm.mut_rate * 4294967296.0);   // exact scaling by 2^32
    flow_gap_params(w.mut_thr, &w.gap_r, &w.gap_s);
    w.lg = reinterpret_cast<const uint32_t *>(c->tab.d_flow.get() + 64);      // (behind the flow order: made in dwgsim_hip_create for every context)
    return w;
}

size_t padded_cells(const Group &g) { return (size_t)g.total + CELL_PAD; }

// The state of a group of `padded` cells besides the cells themselves, in bytes: what a restore copies, what clearing the bitmap covers, and (with a little
// slack: reserve_cell_buffers) what is allocated.  The bitmap: one bit per 64-cell chunk, two words more.
size_t view_bytes(size_t padded) { return padded / 2; }
size_t summ_bytes(size_t padded) { return sizeof(uint16_t) * (padded / SUMM_CELLS); }
size_t summ2_bytes(size_t padded) { return sizeof(uint16_t) * (padded / SUMM2_CELLS); }
uint32_t dirty_words(size_t padded) { return (uint32_t)((padded + 32 * SUMM_CELLS - 1) / (32 * SUMM_CELLS)); }
size_t dirty_bytes(size_t padded) { return sizeof(uint32_t) * ((size_t)dirty_words(padded) + 2); }

// Haplotype h's chosen buffers go back to the pristine copies made at upload (the cells: the packed reference)
enum : unsigned { R_CELLS = 1, R_VIEW = 2, R_SUMM = 4, R_SUMM2 = 8, R_ALL = 15 };
int restore_pristine(dwgsim_hip_ctx *c, const Group &g, int h, unsigned what, hipStream_t st)
{
    const GroupMem &M = g.mem;
    const size_t padded = padded_cells(g);
    if (what & R_CELLS) HIPC(c, hipMemcpyAsync(M.d_cells[h].get(), M.d_ref.get(), padded, hipMemcpyDeviceToDevice, st));
    if (what & R_VIEW) HIPC(c, hipMemcpyAsync(M.d_view[h].get(), M.d_refview.get(), view_bytes(padded), hipMemcpyDeviceToDevice, st));
    if (what & R_SUMM) HIPC(c, hipMemcpyAsync(M.d_summ[h].get(), M.d_refsumm.get(), summ_bytes(padded), hipMemcpyDeviceToDevice, st));
    if (what & R_SUMM2) HIPC(c, hipMemcpyAsync(M.d_summ2[h].get(), M.d_refsumm2.get(), summ2_bytes(padded), hipMemcpyDeviceToDevice, st));
    return 0;
}

// no chunk of the group is dirty
int clear_dirty(dwgsim_hip_ctx *c, const Group &g, hipStream_t st)
{
    HIPC(c, hipMemsetAsync(g.mem.d_dirty.get(), 0, dirty_bytes(padded_cells(g)), st));
    return 0;
}

// a span of the walk's counters: filled with a byte on the device; copied to the group's mirror
hipError_t wc_fill(dwgsim_hip_ctx *c, WcSpan s, int byte, hipStream_t st) { return hipMemsetAsync(c->d_wcounters.get() + s.off, byte, s.bytes, st); }
hipError_t wc_fetch(dwgsim_hip_ctx *c, const GroupMem &M, WcSpan s, hipStream_t st) { return hipMemcpyAsync(M.h_wc.get() + s.off, c->d_wcounters.get() + s.off, s.bytes, hipMemcpyDeviceToHost, st); }

// The four insertion tables of haplotype h: the group's device buffer, the host vector of t and the bytes it holds (up: dwgsim_hip_mutate_async; down:
// fetch_mutated_list, which sizes t first)
struct InsTable { void *dev, *host; size_t bytes; };
std::array<InsTable, 4> ins_tables(const GroupMem &M, int h, HostIns &t)
{
    return {{{M.d_ins_pos[h].get(), t.pos.data(), sizeof(int32_t) * t.pos.size()}, {M.d_ins_len[h].get(), t.len.data(), sizeof(uint32_t) * t.len.size()},
             {M.d_ins_off[h].get(), t.off.data(), sizeof(uint32_t) * t.off.size()}, {M.d_ins_bases[h].get(), t.bases.data(), t.bases.size()}}};
}

SegTab seg_tab(const Group &g)
{
    const int n = (int)g.m.size();
    const int32_t *seg = g.mem.d_seg.get<int32_t>();
    SegTab t; t.start = seg; t.len = seg + (n + 1); t.cindex = reinterpret_cast<const uint32_t *>(seg + (2 * n + 1)); t.n = n;
    return t;
}

void fill_haps(const Group &g, HapDev (&hap)[2])
{
    const GroupMem &M = g.mem;
    for (int h = 0; h < 2; ++h) {
        hap[h].cells = M.d_cells[h].get(); hap[h].view = M.d_view[h].get(); hap[h].ins_pos = M.d_ins_pos[h].get<int32_t>(); hap[h].ins_len = M.d_ins_len[h].get<uint32_t>();
        hap[h].ins_off = M.d_ins_off[h].get<uint32_t>(); hap[h].ins_bases = M.d_ins_bases[h].get(); hap[h].n_ins = g.n_ins[h]; hap[h].pos_off = 0;
    }
}

ContigDev group_dev(const Group &g)
{
    ContigDev d;
    fill_haps(g, d.hap);
    d.ref = g.mem.d_ref.get(); d.l = g.total; d.seg = seg_tab(g);
    d.tot4 = nullptr; d.cap_bases[0] = d.cap_bases[1] = 0;
    return d;
}

// the inserted-base pool of haplotype h (its allocation holds 16 bytes more: ensure_ins)
size_t ins_bases_cap(const Group &g, int h) { const size_t cap = g.mem.d_ins_bases[h].cap(); return cap ? cap - 16 : 0; }

// contig handle -> its group and member (nullptr + error text for a handle that is unknown or was dropped)
Group *get_group(dwgsim_hip_ctx_t *c, int contig, int *k = nullptr)
{
    if (!c) return nullptr;
    if (contig < 0 || (size_t)contig >= c->handles.size() || c->handles[(size_t)contig].group < 0) { c->err = "unknown contig handle"; return nullptr; }
    const HandleRef r = c->handles[(size_t)contig];
    Group &g = c->groups[(size_t)r.group];
    if (!g.alive) { c->err = "unknown contig handle"; return nullptr; }
    if (k) *k = r.k;
    return &g;
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// What the device self-tests (dwgsim_hip_selftest_*) share: n zeroed u64 words on `device`, run(words) launches on the null stream (0, or an error code), the words come back in out
template <class Run> int selftest_words(int device, size_t n, uint64_t *out, Run run)
{
    if (!out || hipSetDevice(device) != hipSuccess) return DWGSIM_HIP_ERR_DEVICE;
    DevMem d;
    if (d.reserve(n * sizeof(uint64_t), n * sizeof(uint64_t)) != hipSuccess) return DWGSIM_HIP_ERR_NOMEM;
    hipMemset(d.get(), 0, n * sizeof(uint64_t));
    if (const int rc = run(d.get<uint64_t>())) return rc;
    const hipError_t e = hipMemcpy(out, d.get(), n * sizeof(uint64_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? DWGSIM_HIP_OK : DWGSIM_HIP_ERR_DEVICE;
}

} // namespace

extern "C" {

void dwgsim_hip_params_default(dwgsim_hip_params_t *p)
{
    memset(p, 0, sizeof(*p));
    p->e_start[0] = p->e_end[0] = p->e_start[1] = p->e_end[1] = 0.02;
    p->dist = 500; p->std_dev = 50; p->N = -1; p->C = 100;
    p->length[0] = p->length[1] = 70;
    p->mut_rate = 0.001; p->mut_freq = 0.5; p->indel_frac = 0.1; p->indel_extend = 0.3; p->indel_min = 1;
    p->rand_read = 0.05; p->seed = -1; p->fixed_quality = -1; p->quality_std = 2.0;
}

#define CHK(v, lo, hi, nm) do { if ((v) < (lo) || (hi) < (v)) { if (msg) snprintf(msg, cap, "Error: command line option %s was out of range\n", nm); return DWGSIM_HIP_ERR_ARG; } } while (0)

int dwgsim_hip_params_check(const dwgsim_hip_params_t *p, char *msg, size_t cap)
{
    if (msg && cap) msg[0] = 0;
    CHK(p->is_inner, 0, 1, "-i"); CHK(p->dist, 0, INT32_MAX, "-d"); CHK(p->std_dev, 0, INT32_MAX, "-s");
    if (p->N < 0 && p->C < 0) { if (msg) snprintf(msg, cap, "Must use one of -N or -C"); return DWGSIM_HIP_ERR_ARG; }
    else if (0 < p->N && 0 < p->C) { if (msg) snprintf(msg, cap, "Cannot use both -N or -C"); return DWGSIM_HIP_ERR_ARG; }
    else if (0 < p->N) { CHK(p->N, 1, INT32_MAX, "-N"); CHK(p->C, INT32_MIN, -1, "-C"); }
    else { CHK(p->N, INT32_MIN, -1, "-N"); CHK(p->C, 0, INT32_MAX, "-C"); }
    CHK(p->length[0], 1, INT32_MAX, "-1"); CHK(p->length[1], 0, INT32_MAX, "-2");
    for (int i = 0; i < 2; ++i) {      // dwgsim_opt.c:329-344
        if (p->e_start[i] < 0.0 || 1.0 < p->e_start[i]) { if (msg) snprintf(msg, cap, "End %s: the start error is out of range (-e)\n", i ? "two" : "one"); return DWGSIM_HIP_ERR_ARG; }
        if (p->e_end[i] < 0.0 || 1.0 < p->e_end[i]) { if (msg) snprintf(msg, cap, "End %s: the end error is out of range (-e)\n", i ? "two" : "one"); return DWGSIM_HIP_ERR_ARG; }
        if (p->data_type == 2 && p->e_end[i] != p->e_start[i]) { if (msg) snprintf(msg, cap, "End %s: a uniform error rate must be given for Ion Torrent data\n", i ? "two" : "one"); return DWGSIM_HIP_ERR_ARG; }
    }
    CHK(p->mut_rate, 0, 1.0, "-r"); CHK(p->indel_frac, 0, 1.0, "-R"); CHK(p->indel_extend, 0, 1.0, "-X");
    CHK(p->indel_min, 1, INT32_MAX, "-I"); CHK(p->data_type, 0, 2, "-c"); CHK(p->strandedness, 0, 2, "-S");
    CHK(p->read_one_strand, 0, 2, "-A"); CHK(p->max_n, 0, INT32_MAX, "-n"); CHK(p->rand_read, 0, 1.0, "-y");
    if (p->data_type == 2 && !p->flow_order) { if (msg) snprintf(msg, cap, "Error: command line option -f is required\n"); return DWGSIM_HIP_ERR_ARG; }
    CHK(p->use_base_error, 0, 1, "-B"); CHK(p->is_hap, 0, 1, "-H");
    if (p->fixed_quality < -1 || p->fixed_quality > 255) { if (msg) snprintf(msg, cap, "Error: command line option -q requires one character\n"); return DWGSIM_HIP_ERR_ARG; }      // (-1: none; dwgsim_opt.c:364-367)
    CHK(p->quality_std, 0, INT32_MAX, "-Q"); CHK(p->reads_output_type, 0, 2, "-o");
    // (not checked by the reference, which treats every other -M as 0 and every non-zero -a as set; the library wants them clean)
    CHK(p->output_type, 0, 2, "-M"); CHK(p->amplicons, 0, 1, "-a");
    if (p->data_type == 2) {       // dwgsim_opt.c:396-413
        const size_t F = strlen(p->flow_order);
        bool has[4] = {false, false, false, false};
        for (size_t i = 0; i < F; ++i) { const uint8_t c = nt4((unsigned char)p->flow_order[i]); if (c < 4) has[c] = true; }
        bool only_acgt = true; for (size_t i = 0; i < F; ++i) if (nt4((unsigned char)p->flow_order[i]) >= 4) only_acgt = false;
        if (F == 0 || F > 64 || !only_acgt || !(has[0] && has[1] && has[2] && has[3])) { if (msg) snprintf(msg, cap, "dwgsim-hip: the flow order (-f) must hold 1..64 flows and contain all of A, C, G, T\n"); return DWGSIM_HIP_ERR_UNSUP; }
    }
    if (p->seed < 0) { if (msg) snprintf(msg, cap, "dwgsim-hip: the seed must be resolved (>= 0) before the context is created\n"); return DWGSIM_HIP_ERR_ARG; }
    return DWGSIM_HIP_OK;
}

int64_t dwgsim_hip_pairs_for_contig(const dwgsim_hip_params_t *p, int64_t l, uint64_t tot_len, int is_last_contig, int64_t n_sim_so_far)
{
    int64_t n_pairs = 0;
    const int size0 = p->length[0], size1 = p->length[1];
    if (is_last_contig && p->C < 0) n_pairs = p->N - n_sim_so_far;                                  // dwgsim.c:535-537
    else if (0 < p->N) {                                                                            // :582-586
        n_pairs = (int64_t)(uint64_t)((long double)l / tot_len * p->N + 0.5);
        if (p->N - n_sim_so_far < n_pairs) n_pairs = p->N - n_sim_so_far;
    } else n_pairs = (int64_t)(uint64_t)(l * p->C / ((long double)(size0 + size1)) / (1.0 - p->rand_read) + 0.5);   // :589
    const int max_len = size0 > size1 ? size0 : size1;
    if (p->amplicons == 1) { if (l < max_len) return DWGSIM_HIP_SKIP_AMPLICON; }                                          // #2 :596-603
    else if (0 < size1 && l < p->dist + 3 * p->std_dev) return DWGSIM_HIP_SKIP_SHORT_INSERT;                                 // #3 :605-611
    else if (l < size0 || (0 < size1 && l < size1)) return DWGSIM_HIP_SKIP_SHORT_READ;                                     // #4 :612-618
    return n_pairs < 0 ? DWGSIM_HIP_SKIP_NO_PAIRS : n_pairs;
}

int dwgsim_hip_device_numa_node(int device)
{
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *q = bus; *q; ++q) *q = (char)tolower((unsigned char)*q);      // sysfs spells the bus id in lower case
    char path[160]; snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

int dwgsim_hip_device_info(int device, char *name, size_t cap, int *n_cu, size_t *hbm_bytes)
{
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device) != hipSuccess) return DWGSIM_HIP_ERR_DEVICE;
    if (name && cap) snprintf(name, cap, "%s (%s)", pr.name, pr.gcnArchName);
    if (n_cu) *n_cu = pr.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = pr.totalGlobalMem;
    return DWGSIM_HIP_ABI_VERSION;
}

int dwgsim_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int dwgsim_hip_failseg_join(uint64_t acc[4], const uint64_t next[4])      // the same monoid as failseg_join in dw_simulate.hip
{
    const uint64_t aP = acc[0], aS = acc[1], aR = acc[2], aB = acc[3], bP = next[0], bS = next[1], bR = next[2], bB = next[3];
    acc[3] = (aB | bB | ((aR && aS + bP > (uint64_t)MAX_ATTEMPTS) ? 1u : 0u)) ? 1 : 0;
    acc[0] = aR ? aP : aP + bP;
    acc[1] = bR ? bS : aS + bS;
    acc[2] = (aR | bR) ? 1 : 0;
    return (acc[3] || acc[0] > (uint64_t)MAX_ATTEMPTS || acc[1] > (uint64_t)MAX_ATTEMPTS) ? 1 : 0;
}

void dwgsim_hip_shard_range(uint64_t n_pairs, int rank, int world, uint64_t *first, uint64_t *n)
{
    if (world < 1) world = 1;
    if (rank < 0) rank = 0;
    const uint64_t base = n_pairs / (uint64_t)world, rem = n_pairs % (uint64_t)world, r = (uint64_t)rank;
    if (first) *first = r * base + (r < rem ? r : rem);
    if (n) *n = base + (r < rem ? 1 : 0);
}

int64_t dwgsim_hip_group_layout(const int64_t *lens, int n, int64_t *starts)
{
    int64_t at = 0;
    for (int k = 0; k < n; ++k) {
        if (!lens || lens[k] < 0) return -1;
        at = align_up(at, GROUP_ALIGN);
        if (starts) starts[k] = at;
        at += lens[k];
    }
    return align_up(at, 16);
}

// Ion Torrent: room for a read after the flow model.  Every empty flow in front of a base inserts Geometric(e) bases, and inserted bases are
// examined again.  How many empty flows a base has in front of it is a property of the flow order: m = the mean distance from a flow to the next
// flow of a given base (about 2.5 for the usual 32-flow orders, 1.5 for TACG, but 15 for an order that keeps three bases away for 37 flows).  The
// mean growth is g = m e / (1 - e) per base, with the cascade 1 / (1 - g); two and a half times that (m is taken as at least 3, twice what the
// usual orders have) plus slack keeps overflow out of reach for realistic error rates -- and what does overflow is run again with twice the room
// (dwgsim_hip_wait), never written out of bounds.  The room is LDS (dw_read.hpp flow_errors: one in-place buffer of cap / 4 bytes per lane), spent sparingly.
static int flow_read_capacity(int len, double e, const std::vector<uint8_t> &flow)
{
    const double ec = !(e > 0) ? 0 : e > 0.9 ? 0.9 : e;       // (NaN, e.g. -B with -e 0: no flow errors at all)
    double m = 3.0;
    const int F = (int)flow.size();
    if (F > 0) {
        double sum = 0;
        for (int f = 0; f < F; ++f) for (uint8_t b = 0; b < 4; ++b) { int k = 0, g = f; while (flow[(size_t)g] != b && k < F) { ++k; g = g + 1 == F ? 0 : g + 1; } sum += k; }
        m = sum / (4.0 * F);
        if (m < 3.0) m = 3.0;
    }
    double g = m * ec / (1.0 - ec);
    g = g / (1.0 - (g < 0.75 ? g : 0.75));
    return len + 32 + (int)(len * 2.5 * g);
}

// Ion Torrent: the read capacity of a job before flow_cap_mult -- "flow_cap" (tests), or flow_read_capacity of the longer read end at the larger error rate
static int flow_base_capacity(const dwgsim_hip_ctx *c)
{
    const int lmax = c->prm.length[0] > c->prm.length[1] ? c->prm.length[0] : c->prm.length[1];
    const double emax = c->prm.e_start[0] > c->prm.e_start[1] ? c->prm.e_start[0] : c->prm.e_start[1];
    return c->dbg.flow_cap_forced > 0 ? c->dbg.flow_cap_forced : flow_read_capacity(lmax, emax, c->tab.flow);
}

static int set_err(int *err, int v) { if (err) *err = v; return v; }

// ---- dwgsim_hip_create, step by step (each fills one part of the context and returns 0 or the error code; create runs them in order) ----

// The four streams every context has, and the events that are not a slot's or a group's
static int open_streams(dwgsim_hip_ctx *c)
{
    HIPC(c, hipSetDevice(c->device));
    // What prepares the NEXT group (upload, walk, random-read count: walk stream) runs at the batches' own priority.  Rounds 3-5 put it below them ("fills the
    // thinning tail of every launch instead of taking slots"): its fifteen small kernels then ran one after the other in the gap between two k_simulate launches --
    // 0.07 of the 0.46 ms of an E. coli-sized step.  At equal priority they slip in as slots fall free while the big kernel runs and are done when it ends: E. coli-sized
    // 1 146-1 159 against 980-1 060 M pairs/s, chr20-sized / whole genome / N-rank weak lines unchanged (profiles/r06_bench_lines_final.txt 15).
    int prio_least = 0, prio_greatest = 0;
    HIPC(c, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    // (DWGSIM_HIP_WALK_PRIO=low|mid|above: analysis -- the walk stream below the batches (rounds 3-5), between the two, or the batches below the walk)
    int prio_walk = prio_greatest, prio_batch = prio_greatest;
    if (const char *e = getenv("DWGSIM_HIP_WALK_PRIO")) {
        prio_walk = !strcmp(e, "high") || !strcmp(e, "above") ? prio_greatest : !strcmp(e, "mid") ? (prio_least + prio_greatest) / 2 : prio_least;
        if (!strcmp(e, "above")) prio_batch = prio_least;
    }
    HIPC(c, c->stream.create(prio_batch));
    HIPC(c, c->copy_stream.create(prio_greatest));
    HIPC(c, c->walk_stream.create(prio_walk));
    HIPC(c, c->count_stream.create(prio_walk));
    HIPC(c, c->ev_up.create()); HIPC(c, c->ev_cnt0.create()); HIPC(c, c->ev_cnt1.create());
    return 0;
}

// The counter blocks of the context and of each slot, the chain words (zeroed), and each slot's events
static int reserve_counter_blocks(dwgsim_hip_ctx *c)
{
    const size_t cnt_bytes = N_COUNTERS * sizeof(uint64_t);
    auto counters = [&](Counters &k) -> int { HIPC(c, reserve(c, k.d, cnt_bytes, cnt_bytes)); HIPC(c, k.h.reserve(cnt_bytes, cnt_bytes)); return 0; };
    if (int rc = counters(c->counters)) return rc;
    HIPC(c, reserve(c, c->d_wcounters, sizeof(WalkCounters), sizeof(WalkCounters)));
    if (int rc = counters(c->pcounters)) return rc;
    HIPC(c, reserve(c, c->d_chain, 4 * sizeof(uint64_t), 4 * sizeof(uint64_t)));
    HIPC(c, hipMemset(c->d_chain.get(), 0, 4 * sizeof(uint64_t)));
    for (Slot &sl : c->slot) {
        if (int rc = counters(sl.counters)) return rc;
        HIPC(c, reserve(c, sl.d_rerun_chain, 2 * sizeof(uint64_t), 2 * sizeof(uint64_t)));
        HIPC(c, sl.ev_k0.create()); HIPC(c, sl.ev_k1.create()); HIPC(c, sl.ev_end.create()); HIPC(c, sl.ev_done.create()); HIPC(c, sl.ev_fetched.create());
    }
    return 0;
}

// The flow order (64 bytes) and, behind it, the log2 table the flow model's gap draws interpolate in (dw_kernels.hpp flow_log2_table)
static int upload_flow_order(dwgsim_hip_ctx *c)
{
    std::vector<uint8_t> fl(64 + sizeof(uint32_t) * FLOW_LG_ENTRIES, 4); for (size_t i = 0; i < c->tab.flow.size() && i < 64; ++i) fl[i] = c->tab.flow[i];
    flow_log2_table(reinterpret_cast<uint32_t *>(fl.data() + 64));
    return upload(c, c->tab.d_flow, fl.data(), fl.size());
}

struct CalibRun { int mult; bool outgrown; int32_t n_err, counts; };      // the room the reads needed (times flow_read_capacity), whether one still outgrew it; int32 accumulators as in the reference

// -B, the buffer mechanics: the 10^6 random reads of read end i at flow error rate e, run with room doubled until no read outgrows its buffers
static int calibrate_end(dwgsim_hip_ctx *c, int i, double e, CalibRun *r)
{
    const int len = c->prm.length[i];
    CalibArgs ca;
    ca.seed = (uint32_t)c->prm.seed; ca.end = i; ca.len = len; ca.n_reads = 1000000;       // ERROR_RATE_NUM_RANDOM_READS, dwgsim_opt.h:5
    ca.thr = !(e > 0) ? 0 : e >= 1.0 ? 0x100000000ull : (uint64_t)ceil(e * 4294967296.0);
    flow_gap_params(ca.thr, &ca.gap_r, &ca.gap_s);
    ca.flow = c->tab.d_flow.get(); ca.flow_len = (int32_t)c->tab.flow.size();
    // a read that outgrows its buffers: once more with twice the room (the reference doubles its buffers, dwgsim.c:296-311) -- by the rule of
    // dwgsim_hip_wait: up to FLOW_CAP_MAX bases per read.  The scratch holds a CHUNK of the 10^6 reads (at most ~2 GiB), so the room a read
    // may take does not depend on how many reads there are (round 5 stopped at 16 x: -B then refused flow orders the simulate path handles)
    const int64_t base_cap = flow_read_capacity(len, e, c->tab.flow);
    int mult = 1;
    for (;; mult *= 2) {
        ca.lds_words = (int32_t)((base_cap * mult + 15) / 16);       // the flow model's one buffer per lane: 16 bases per word
        ca.stack_words = std::min(FLOW_STACK_WORDS * mult, FLOW_STACK_WORDS_MAX);
        const size_t per_block = (size_t)ca.lds_words * PAIRS_PER_BLOCK * sizeof(uint32_t);
        const size_t nblk_all = (size_t)((ca.n_reads + PAIRS_PER_BLOCK - 1) / PAIRS_PER_BLOCK);
        const size_t nblk = std::max<size_t>(1, std::min(nblk_all, ((size_t)2 << 30) / per_block));
        ca.chunk_reads = (uint64_t)nblk * PAIRS_PER_BLOCK;
        if (int rc = ensure(c, c->flow_scratch, per_block * nblk)) return rc;
        ca.scratch = c->flow_scratch.get<uint32_t>(); ca.counters = c->counters.dev();
        HIPC(c, hipMemsetAsync(c->counters.dev(), 0, N_COUNTERS * sizeof(uint64_t), c->stream.get()));
        for (ca.first_read = 0; ca.first_read < ca.n_reads; ca.first_read += ca.chunk_reads) launch_calibrate(c->stream.get(), ca);
        HIPC(c, hipMemcpyAsync(c->counters.host(), c->counters.dev(), N_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream.get()));
        HIPC(c, hipStreamSynchronize(c->stream.get()));
        if (!(c->counters.host()[STATUS_COUNTER] & FLOW_ROOM_BIT) || base_cap * (int64_t)mult * 2 > (int64_t)FLOW_CAP_MAX) break;
    }
    r->mult = mult; r->outgrown = (c->counters.host()[STATUS_COUNTER] & FLOW_ROOM_BIT) != 0; r->n_err = (int32_t)c->counters.host()[CALIB_ERR_COUNTER]; r->counts = (int32_t)c->counters.host()[CALIB_LEN_COUNTER];
    return 0;
}

// -B (dwgsim_opt.c:415-457): rescale the flow error so that the per-base error rate of 10^6 random reads matches -e.  Reads that outgrow their buffers
// are reported as DWGSIM_HIP_ERR_FAILED: an option set, not the device.
static int calibrate_base_error(dwgsim_hip_ctx *c)
{
    if (c->prm.data_type != 2 || !c->prm.use_base_error) return 0;
    double sf = 0.0;
    for (int i = 0; i < 2; ++i) {
        const int len = c->prm.length[i];
        if (len <= 0) continue;
        fprintf(stderr, "[dwgsim_core] Updating error rate for end %d\n", i + 1);
        if (0 < i && len == c->prm.length[1 - i]) {
            c->prm.e_start[i] = c->prm.e_start[1 - i]; c->prm.e_end[i] = c->prm.e_end[1 - i];
            fprintf(stderr, "[dwgsim_core] Using scaling factor from previous end\n[dwgsim_core] Updated with scaling factor %.5lf\n", sf);
            continue;
        }
        const double e = c->prm.e_start[i];
        CalibRun r;
        if (int rc = calibrate_end(c, i, e, &r)) return rc;
        // the job's reads will need the room the calibration's needed: start there instead of running the first overflowing batch twice
        if (r.mult > c->flow_cap_mult) c->flow_cap_mult = r.mult;
        if (r.outgrown) { c->err = "-B calibration: a read outgrew its flow-space buffer (the flow model's growth at this error rate and flow order: INTEGRATION.md)"; return DWGSIM_HIP_ERR_FAILED; }
        sf = e / (r.n_err / (1.0 * r.counts));
        c->prm.e_end[i] *= sf; c->prm.e_start[i] = c->prm.e_end[i];
        fprintf(stderr, "[dwgsim_core] Updated with scaling factor %.5lf!\n", sf);
    }
    return 0;
}

// Read end j's per-position error thresholds and base qualities (dwgsim_opt.c:459-460, dwgsim.c:237, :906-910)
static int upload_error_tables(dwgsim_hip_ctx *c, int j)
{
    auto &T = c->tab;
    const int n = c->prm.length[j];
    if (n <= 0) return 0;
    T.e_by[j] = (c->prm.e_end[j] - c->prm.e_start[j]) / n;
    std::vector<uint64_t> thr((size_t)n); std::vector<int8_t> qb((size_t)n);
    for (int i = 0; i < n; ++i) {
        const double ei = c->prm.e_start[j] + T.e_by[j] * i;
        thr[(size_t)i] = !(ei > 0) ? 0 : ei >= 1.0 ? 0x100000000ull : (uint64_t)ceil(ei * 4294967296.0);   // u = w * 2^-32 < ei  <=>  w < ceil(ei * 2^32) (exact: scaling by 2^32 is exact)
        char q;
        if (ei > 0) q = (char)((int)(-10.0 * log(ei) / log(10.0) + 0.499) + '!'); else q = 40 + '!';
        qb[(size_t)i] = (int8_t)q;
    }
    if (int rc = upload(c, T.d_thr[j], thr.data(), sizeof(uint64_t) * (size_t)n)) return rc;
    // packed table: n entries, then the last one repeated (>= 8 copies), the same word count for both read ends
    const int lmax = c->prm.length[0] > c->prm.length[1] ? c->prm.length[0] : c->prm.length[1];
    T.qb_words = (lmax + 4 + 3) / 4 + 2;      // (a block of the quality stream looks at eight positions: three words from any position <= lmax)
    std::vector<int8_t> padded((size_t)T.qb_words * 4, qb[(size_t)n - 1]);
    memcpy(padded.data(), qb.data(), (size_t)n);
    if (int rc = upload(c, T.d_qbase[j], padded.data(), padded.size())) return rc;
    std::vector<uint32_t> t32(((size_t)n + 7) / 8 * 8, 0u);
    for (int i = 0; i < n; ++i) {
        if (thr[(size_t)i] >= 0x100000000ull) { t32[(size_t)i] = 0xFFFFFFFFu; T.e_full = 1; }
        else t32[(size_t)i] = (uint32_t)thr[(size_t)i];
    }
    if (T.e_full) for (int i = 0; i < n; ++i) if (thr[(size_t)i] == 0xFFFFFFFFull) { c->err = "an error rate within 2^-32 of (but not equal to) 1 next to one equal to 1 is not representable"; return DWGSIM_HIP_ERR_DEVICE; }
    return upload(c, T.d_thr32[j], t32.data(), sizeof(uint32_t) * t32.size());
}

// '@' + "[prefix_]rand", zero padded to >= 256 + 16 bytes (the kernel stages 128 bytes in LDS)
static int upload_rand_name(dwgsim_hip_ctx *c)
{
    std::string rf = c->read_prefix.empty() ? std::string("rand") : c->read_prefix + "_rand";
    c->tab.rand_fixed_len = (int32_t)rf.size();
    std::string rbuf = "@" + rf; rbuf.resize(rbuf.size() < 256 ? 272 : rbuf.size() + 16, '\0');
    return upload(c, c->tab.d_rand_fixed, rbuf.data(), rbuf.size());
}

dwgsim_hip_ctx_t *dwgsim_hip_create(const dwgsim_hip_params_t *p, int device, int *err)
{
    char msg[512];
    int rc = dwgsim_hip_params_check(p, msg, sizeof msg);
    if (rc != DWGSIM_HIP_OK) { fprintf(stderr, "%s", msg); set_err(err, rc); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        fprintf(stderr, "dwgsim-hip: no usable HIP device (requested %d of %d); the hot path has no CPU fallback\n", device, ndev);
        set_err(err, DWGSIM_HIP_ERR_DEVICE); return nullptr;
    }
    dwgsim_hip_ctx *c = new dwgsim_hip_ctx();
    c->prm = *p;
    if (p->read_prefix) c->read_prefix = p->read_prefix;
    if (p->data_type == 2) for (const char *q = p->flow_order; *q; ++q) c->tab.flow.push_back(nt4((unsigned char)*q));
    c->prm.read_prefix = nullptr; c->prm.flow_order = nullptr;
    c->device = device;
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess) c->n_cu = pr.multiProcessorCount; if (c->n_cu <= 0) c->n_cu = 256; }
    auto fail = [&](int code) { fprintf(stderr, "dwgsim-hip: context initialisation failed: %s\n", c->err.c_str()); set_err(err, code); dwgsim_hip_destroy(c); return (dwgsim_hip_ctx *)nullptr; };
    if ((rc = open_streams(c))) return fail(rc);
    if ((rc = reserve_counter_blocks(c))) return fail(rc);
    if ((rc = upload_flow_order(c))) return fail(rc);
    if ((rc = calibrate_base_error(c))) return fail(rc);
    for (int j = 0; j < 2; ++j) if ((rc = upload_error_tables(c, j))) return fail(rc);
    if ((rc = upload_rand_name(c))) return fail(rc);
    set_err(err, DWGSIM_HIP_OK);
    return c;
}

// Not part of the drop-in ABI (include/dwgsim_hip.h): a device self-test used by tests/test_gpu_parity.py.  Compares the
// range-restricted fp64 division / sqrt / log of the quality path with the compiler's general forms on n operand sets;
// out[0..2] = bitwise differences (division, sqrt, log), out[3] = comparisons made.
extern "C" int dwgsim_hip_selftest_fp64(int device, uint32_t seed, uint64_t n, uint64_t *out)
{
    return selftest_words(device, 4, out, [&](uint64_t *d) { launch_selftest_fp64(nullptr, seed, n, d); return 0; });
}

// Not part of the drop-in ABI either: the number formatters of the name line (dw_read.hpp put_dec / put_hex) against one division per digit, on the
// values first + i * stride, i < n (dw_simulate.hip k_selftest_text).  out[0] / out[1] = decimal / hexadecimal texts that differ, out[2] = values compared.
extern "C" int dwgsim_hip_selftest_text(int device, uint64_t first, uint64_t n, uint64_t stride, uint64_t *out)
{
    return selftest_words(device, 4, out, [&](uint64_t *d) { launch_selftest_text(nullptr, first, n, stride, d); return 0; });
}

// Not part of the drop-in ABI either: the gap draw geom_gap at threshold thr (0 < thr < 2^32) on the words [first, first + n), with the R, s and log2 table
// of the product's own host functions (dw_kernels.hpp flow_gap_params, flow_log2_table) -- dw_simulate.hip k_selftest_gap.  chg (g_cnt words, host
// memory): chg[k] = the first word w in (first, first + n) whose G is below g_lo + k, 0 where no word of the range is (the whole range: #{w : G(w) >= g}).
// out[0] = words where G increases with w, out[1] = words at the clip 0x3FFFFFFF, out[2] = words evaluated, out[3] = G of the last word.
extern "C" int dwgsim_hip_selftest_gap(int device, uint64_t thr, uint32_t first, uint64_t n, uint32_t g_lo, uint32_t g_cnt, uint32_t *chg, uint64_t *out)
{
    if (!out || (g_cnt && !chg) || thr == 0 || thr >= 0x100000000ull || n == 0 || (uint64_t)first + n > 0x100000000ull) return DWGSIM_HIP_ERR_ARG;
    uint32_t lg[FLOW_LG_ENTRIES];
    flow_log2_table(lg);
    uint64_t R; int32_t sR;
    flow_gap_params(thr, &R, &sR);
    DevMem d_lg, d_chg;
    const size_t chg_bytes = (size_t)g_cnt * sizeof(uint32_t), chg_alloc = chg_bytes ? chg_bytes : 4;
    const int rc = selftest_words(device, 4, out, [&](uint64_t *d) {
        if (d_lg.reserve(sizeof lg, sizeof lg) != hipSuccess || d_chg.reserve(chg_alloc, chg_alloc) != hipSuccess) return DWGSIM_HIP_ERR_NOMEM;
        hipMemset(d_chg.get(), 0, chg_alloc);
        hipMemcpy(d_lg.get(), lg, sizeof lg, hipMemcpyHostToDevice);
        launch_selftest_gap(nullptr, d_lg.get<uint32_t>(), R, sR, first, n, g_lo, g_cnt, d_chg.get<uint32_t>(), d);
        return DWGSIM_HIP_OK;
    });
    if (rc != DWGSIM_HIP_OK || !chg_bytes) return rc;
    return hipMemcpy(chg, d_chg.get(), chg_bytes, hipMemcpyDeviceToHost) == hipSuccess ? DWGSIM_HIP_OK : DWGSIM_HIP_ERR_DEVICE;
}

// Not part of the drop-in ABI either: self-test of the lazy quality normals (dw_simulate.hip k_selftest_lazy).  out[0..4] = counters of the
// comparison with the exact form on the n tries w = first, first + 1, ... (n = 2^32: EVERY try) at quality_std = sigma, out[5] = max
// |estimate - exact| / eps, out[6..8] = worst error of v_log_f32 / v_rcp_f32 / v_sqrt_f32 over EVERY float of their operand ranges, in units of
// the bounds the error budget assumes (doubles).
extern "C" int dwgsim_hip_selftest_lazy(int device, uint32_t first, uint64_t n, double sigma, int exhaustive, uint64_t *out)
{
    float qk, qeps, qlmin; int32_t qnear1;
    lazy_quality_params(sigma, &qk, &qeps, &qlmin, &qnear1);
    return selftest_words(device, 12, out, [&](uint64_t *d) {
        launch_selftest_lazy(nullptr, 0, first, n, sigma, qk, qeps, qlmin, qnear1, d);
        if (exhaustive) {
            launch_selftest_lazy(nullptr, 1, 0, 0x3F800000u - 0x30800000u, 0, 0, 0, 0, 0, d);           // [2^-30, 1)
            launch_selftest_lazy(nullptr, 2, 0, 0x4E800000u - 0x3F800000u + 1u, 0, 0, 0, 0, 0, d);      // [1, 2^30]
            launch_selftest_lazy(nullptr, 3, 0, 0x42000000u - 0x2B000000u, 0, 0, 0, 0, 0, d);           // [2^-41, 2^5)
        }
        return 0;
    });
}

// The streams that exist are waited for here, by name: the members' destructors (dwgsim_hip_ctx) only give handles and memory back
void dwgsim_hip_destroy(dwgsim_hip_ctx_t *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    for (const DevStream *s : {&c->stream, &c->copy_stream, &c->walk_stream, &c->count_stream, &c->hap_stream}) if (*s) hipStreamSynchronize(s->get());
    delete c;
}

const char *dwgsim_hip_last_error(const dwgsim_hip_ctx_t *c) { return c ? c->err.c_str() : "no context"; }

int dwgsim_hip_get_params(const dwgsim_hip_ctx_t *c, dwgsim_hip_params_t *out)
{
    if (!c || !out) return DWGSIM_HIP_ERR_ARG;
    *out = c->prm;      // (read_prefix / flow_order were cleared when the context took its copies)
    return DWGSIM_HIP_OK;
}

static bool in_host_registry(const void *p);
static bool is_page_locked(const void *p)
{
    if (in_host_registry(p)) return true;      // (dwgsim_hip_host_alloc)
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost) return true;
    (void)hipGetLastError();      // pageable memory: the query reports an error that must not stick
    return false;
}

// ---- dwgsim_hip_add_contigs, step by step (build_group runs them in order; what they enqueue goes to the walk stream) ----

// A free group slot, reset, with the memory of a dropped group if one is large enough for `want` cells (the smallest such; none more than four times too large)
static int take_group(dwgsim_hip_ctx_t *c, size_t want)
{
    int gid = -1;
    for (size_t i = 0; i < c->groups.size(); ++i) if (!c->groups[i].alive) { gid = (int)i; break; }
    if (gid < 0) { c->groups.emplace_back(); gid = (int)c->groups.size() - 1; }
    Group &g = c->groups[(size_t)gid];
    g = Group();
    int best = -1;
    for (size_t i = 0; i < c->pool.size(); ++i) {
        const size_t cap = c->pool[i].d_ref.cap();
        if (cap >= want && cap <= 4 * want + (1u << 20) && (best < 0 || cap < c->pool[(size_t)best].d_ref.cap())) best = (int)i;
    }
    if (best >= 0) { g.mem = std::move(c->pool[(size_t)best]); c->pool.erase(c->pool.begin() + best); }
    return gid;
}

// The events, the counter mirror and the buffers of cells of a group of `padded` cells.  The buffers of cells go and come together (d_ref's capacity stands
// for all of them); views and summaries hold 32 bytes more than a restore copies.
static int reserve_cell_buffers(dwgsim_hip_ctx_t *c, GroupMem &M, size_t padded)
{
    HIPC(c, M.ev_walk.create()); HIPC(c, M.ev_walk0.create());
    HIPC(c, M.h_wc.reserve(sizeof(WalkCounters), sizeof(WalkCounters)));
    if (M.d_ref.cap() >= padded) return 0;
    const size_t view = view_bytes(padded) + 32, summ = summ_bytes(padded) + 32, summ2 = summ2_bytes(padded) + 32;
    const struct { DevMem *buf; size_t bytes; } cellbufs[] = {
        {&M.d_ref, padded}, {&M.d_cells[0], padded}, {&M.d_view[0], view}, {&M.d_summ[0], summ}, {&M.d_summ2[0], summ2},
        {&M.d_cells[1], padded}, {&M.d_view[1], view}, {&M.d_summ[1], summ}, {&M.d_summ2[1], summ2},
        {&M.d_refview, view}, {&M.d_refsumm, summ}, {&M.d_refsumm2, summ2}, {&M.d_dirty, dirty_bytes(padded)}};
    for (const auto &b : cellbufs) b.buf->reset();
    for (const auto &b : cellbufs) HIPC(c, reserve(c, *b.buf, b.bytes, b.bytes));
    return 0;
}

// The sequence goes up into c->up_ascii.  One copy when the caller's buffers already are the group layout inside ONE page-locked
// allocation (ascii[k] = ascii[0] + start[k], zero bytes between the contigs): nothing is staged and the call need not wait -- the
// buffers must then stay as they are until dwgsim_hip_mutate_wait returned.  A few contigs: one copy each into a zeroed device buffer.
// Many: packed into page-locked staging first (one copy instead of thousands).  must_wait: the call may only return once the walk
// stream has read the caller's buffers (every form but the first).
static int upload_sequence(dwgsim_hip_ctx_t *c, int n, const uint8_t *const *ascii, const int64_t *lens, const int64_t *starts, int64_t total, size_t padded, bool &must_wait)
{
    if (ensure(c, c->up_ascii, padded)) return DWGSIM_HIP_ERR_DEVICE;
    uint8_t *d_ascii = c->up_ascii.get();
    must_wait = true;
    bool laid_out = true;
    for (int k = 0; k < n && laid_out; ++k) if (lens[k] > 0 && ascii[k] != ascii[0] + starts[k]) laid_out = false;
    if (laid_out && n > 0 && ascii[0] && is_page_locked(ascii[0])) {
        HIPC(c, hipMemcpyAsync(d_ascii, ascii[0], (size_t)total, hipMemcpyHostToDevice, c->walk_stream.get()));
        HIPC(c, hipMemsetAsync(d_ascii + total, 0, padded - (size_t)total, c->walk_stream.get()));
        must_wait = false;
    } else if (n <= 8) {
        HIPC(c, hipMemsetAsync(d_ascii, 0, padded, c->walk_stream.get()));
        for (int k = 0; k < n; ++k) if (lens[k] > 0) HIPC(c, hipMemcpyAsync(d_ascii + starts[k], ascii[k], (size_t)lens[k], hipMemcpyHostToDevice, c->walk_stream.get()));
    } else {
        if (c->up_in_flight) { HIPC(c, hipEventSynchronize(c->ev_up.get())); c->up_in_flight = false; }
        HIPC(c, c->h_up.reserve((size_t)total, (size_t)total + (size_t)total / 4 + 4096));
        uint8_t *h_up = c->h_up.get();
        for (int k = 0; k < n; ++k) {
            const int64_t end = starts[k] + lens[k], next = k + 1 < n ? starts[k + 1] : total;
            if (lens[k] > 0) memcpy(h_up + starts[k], ascii[k], (size_t)lens[k]);
            memset(h_up + end, 0, (size_t)(next - end));
        }
        HIPC(c, hipMemcpyAsync(d_ascii, h_up, (size_t)total, hipMemcpyHostToDevice, c->walk_stream.get()));
        HIPC(c, hipMemsetAsync(d_ascii + total, 0, padded - (size_t)total, c->walk_stream.get()));
        HIPC(c, hipEventRecord(c->ev_up.get(), c->walk_stream.get())); c->up_in_flight = true;
    }
    return 0;
}

// The pristine state, from the uploaded sequence: the packed reference and both haplotypes' cells; the read views and summaries of the unmutated
// group, once -- the pristine copies, and what both haplotypes start from (a walk then rewrites only the chunks it touches); a zeroed bitmap
static int make_pristine(dwgsim_hip_ctx_t *c, const Group &g)
{
    const GroupMem &M = g.mem;
    const int64_t n_cells = (int64_t)padded_cells(g) & ~(int64_t)15;
    uint8_t *ref = M.d_ref.get();
    launch_pack(c->walk_stream.get(), c->up_ascii.get(), ref, M.d_cells[0].get(), M.d_cells[1].get(), n_cells);
    launch_make_view(c->walk_stream.get(), ref, ref, n_cells, g.total, M.d_refview.get(), M.d_view[0].get(), M.d_refsumm.get<uint16_t>(), M.d_summ[0].get<uint16_t>(), M.d_refsumm2.get<uint16_t>(), M.d_summ2[0].get<uint16_t>());
    if (const int rc = restore_pristine(c, g, 1, R_VIEW | R_SUMM | R_SUMM2, c->walk_stream.get())) return rc;
    if (const int rc = clear_dirty(c, g, c->walk_stream.get())) return rc;
    HIPC(c, hipGetLastError());
    return 0;
}

// Segment table, name pool and (-x) target regions of a group: made on the host, uploaded
static int upload_group_tables(dwgsim_hip_ctx_t *c, Group &g)
{
    GroupMem &M = g.mem;
    const int n = (int)g.m.size();
    M.h_seg.assign((size_t)(3 * n + 1), 0);
    for (int k = 0; k < n; ++k) { M.h_seg[(size_t)k] = g.m[(size_t)k].start; M.h_seg[(size_t)(n + 1 + k)] = (int32_t)g.m[(size_t)k].l; M.h_seg[(size_t)(2 * n + 1 + k)] = (int32_t)g.m[(size_t)k].contig_index; }
    M.h_seg[(size_t)n] = (int32_t)g.total;
    if (const int rc = upload_table(c, M.d_seg, M.h_seg, 64)) return rc;
    M.h_names.clear();
    for (Member &m : g.m) {      // '@' + "[prefix_]name", zero padded to >= 256 + 16 bytes (the kernel stages 128 bytes in LDS), entries 16-byte aligned
        const std::string nf = c->read_prefix.empty() ? m.name : c->read_prefix + "_" + m.name;
        m.name_fixed_len = (int32_t)nf.size(); m.name_off = (uint32_t)M.h_names.size();
        if (m.name_fixed_len > g.fixed_max) g.fixed_max = m.name_fixed_len;
        const size_t room = ((nf.size() + 1 < 256 ? 272 : nf.size() + 1 + 16) + 15) & ~(size_t)15;
        M.h_names.resize(M.h_names.size() + room, 0);
        M.h_names[m.name_off] = '@'; memcpy(&M.h_names[m.name_off + 1], nf.data(), nf.size());
    }
    if (const int rc = upload_table(c, M.d_names, M.h_names, 4096)) return rc;
    M.h_reg.clear();
    if (!c->has_regions) return 0;
    for (Member &m : g.m) {      // [starts | ends] of the contig's regions; fragments are placed on their total length
        std::vector<int32_t> st, en; int64_t tot = 0;
        for (size_t q = 0; q < c->regions.contig.size(); ++q) if (c->regions.contig[q] == m.contig_index) { st.push_back((int32_t)c->regions.start[q]); en.push_back((int32_t)c->regions.end[q]); tot += c->regions.end[q] - c->regions.start[q]; }
        m.reg_off = (int32_t)M.h_reg.size(); m.n_reg = (int32_t)st.size(); m.l_place = tot;
        M.h_reg.insert(M.h_reg.end(), st.begin(), st.end()); M.h_reg.insert(M.h_reg.end(), en.begin(), en.end());
    }
    M.h_reg.push_back(0);
    return upload_table(c, M.d_reg, M.h_reg, 64);
}

// Everything a new group needs on the device, enqueued on the walk stream.  A step that fails returns at once: the caller undoes the group.
static int build_group(dwgsim_hip_ctx_t *c, Group &g, const uint8_t *const *ascii, const int64_t *lens, const int64_t *starts)
{
    const int n = (int)g.m.size();
    const size_t padded = padded_cells(g);
    bool must_wait = true;
    if (const int rc = reserve_cell_buffers(c, g.mem, padded)) return rc;
    if (const int rc = upload_sequence(c, n, ascii, lens, starts, g.total, padded, must_wait)) return rc;
    if (const int rc = make_pristine(c, g)) return rc;
    if (const int rc = upload_group_tables(c, g)) return rc;
    // -m / -b / -v: the file's entries for these contigs are resolved now, while the sequence is at hand (mut.c:644-745)
    if (c->has_mutin) for (int k = 0; k < n; ++k) resolve_mutation_input(c->mutin, g.m[(size_t)k].contig_index, ascii[k], lens[k], (uint32_t)c->prm.seed, c->prm.is_hap != 0, g.m[(size_t)k].rc);
    if (must_wait) HIPC(c, hipStreamSynchronize(c->walk_stream.get()));
    return 0;
}

int dwgsim_hip_add_contigs(dwgsim_hip_ctx_t *c, int n, const char *const *names, const uint8_t *const *ascii, const int64_t *lens, const uint32_t *contig_index)
{
    if (!c || n < 1 || !names || !ascii || !lens || !contig_index) { if (c) c->err = "bad contig arguments"; return DWGSIM_HIP_ERR_ARG; }
    for (int k = 0; k < n; ++k) if (!names[k] || (!ascii[k] && lens[k] > 0) || lens[k] < 0 || lens[k] > INT32_MAX) { c->err = "bad contig arguments"; return DWGSIM_HIP_ERR_ARG; }
    std::vector<int64_t> starts((size_t)n);
    const int64_t total = dwgsim_hip_group_layout(lens, n, starts.data());
    if (total < 0 || total > (int64_t)INT32_MAX - 2 * GROUP_ALIGN) { c->err = "dwgsim-hip: the contigs of one group must stay below 2^31 cells in all (add them in smaller groups)\n"; return DWGSIM_HIP_ERR_ARG; }
    HIPC(c, hipSetDevice(c->device));
    const int gid = take_group(c, (size_t)total + CELL_PAD);
    Group &g = c->groups[(size_t)gid];
    g.alive = true; g.total = total; g.first_handle = (int)c->handles.size();
    g.m.resize((size_t)n);
    for (int k = 0; k < n; ++k) { Member &m = g.m[(size_t)k]; m.name = names[k]; m.l = m.l_place = lens[k]; m.contig_index = contig_index[k]; m.start = (int32_t)starts[(size_t)k]; }
    const int rc = build_group(c, g, ascii, lens, starts.data());
    if (rc != 0) { (void)hipStreamSynchronize(c->walk_stream.get()); g = Group(); return rc; }      // no half-built group stays behind a failed call
    for (int k = 0; k < n; ++k) c->handles.push_back(HandleRef{gid, k});
    return g.first_handle;
}

int dwgsim_hip_add_contig(dwgsim_hip_ctx_t *c, const char *name, const uint8_t *ascii, int64_t len, uint32_t contig_index)
{
    return dwgsim_hip_add_contigs(c, 1, &name, &ascii, &len, &contig_index);
}

int dwgsim_hip_drop_contig(dwgsim_hip_ctx_t *c, int contig)
{
    Group *g = get_group(c, contig);
    if (!g) return DWGSIM_HIP_ERR_ARG;
    hipSetDevice(c->device);
    // what may still read the group's memory: the kernels of batches that were enqueued and not waited for (not the whole compute stream: it may
    // already carry batches of the NEXT group -- the job level keeps its three batches in flight across a group's end -- and not the copy stream:
    // copies read the slots' output buffers), and the group's own walk (not the whole walk stream: it may carry the upload and the walk of the next group)
    const int gid = (int)(g - c->groups.data());
    // a batch of the group that was enqueued and not yet waited for: its wait may have to run it AGAIN (an Ion Torrent read that outgrew its buffers,
    // dwgsim_hip_wait), which needs the group -- wait first, then drop (include/dwgsim_hip.h)
    for (int s = 0; s < DWGSIM_HIP_SLOTS; ++s) if (c->slot[s].pending && !c->slot[s].empty && c->slot[s].group == gid) { c->err = "drop_contig: a batch that reads this group has not been waited for (dwgsim_hip_wait first)"; return DWGSIM_HIP_ERR_STATE; }
    if (g->walk_pending) hipEventSynchronize(g->mem.ev_walk.get());
    for (size_t k = 0; k < g->m.size(); ++k) { if (c->chain_contig == g->first_handle + (int)k) c->chain_contig = -1; c->handles[(size_t)g->first_handle + k].group = -1; }
    for (int h = 0; h < 2; ++h) if (c->hap_cur[h] == gid) c->hap_cur[h] = -1;
    // the group's memory waits for the next group (at most three sets are kept: the one that has waited longest goes -- a set that no later
    // group can use, e.g. one more than four times too large, does not stay for the life of the context; round 5 dropped the smallest)
    c->pool.push_back(std::move(g->mem));
    *g = Group();
    if (c->pool.size() > 3) {
        hipStreamSynchronize(c->walk_stream.get());
        c->pool.erase(c->pool.begin());
    }
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_set_regions(dwgsim_hip_ctx_t *c, const char *path, const char *const *names, const int64_t *lens, int n_contigs, uint64_t *total_len)
{
    if (!c || !path || n_contigs < 0 || (n_contigs && (!names || !lens))) { if (c) c->err = "bad regions arguments"; return DWGSIM_HIP_ERR_ARG; }
    if (c->prm.amplicons) { c->err = "Error: cannot use a regions BED file (-x) when simulating amplicons (-a)\n"; return DWGSIM_HIP_ERR_ARG; }
    std::vector<ContigName> tab;
    for (int i = 0; i < n_contigs; ++i) tab.push_back(ContigName{names[i], lens[i]});
    std::string err;
    if (!parse_regions(path, tab, c->regions, err)) { c->err = err; c->has_regions = false; return DWGSIM_HIP_ERR_ARG; }
    c->has_regions = true;
    uint64_t tot = 0;
    for (size_t q = 0; q < c->regions.start.size(); ++q) tot += c->regions.end[q] - c->regions.start[q];
    if (total_len) *total_len = tot;
    return DWGSIM_HIP_OK;
}

int64_t dwgsim_hip_contig_region_length(dwgsim_hip_ctx_t *c, uint32_t contig_index, const uint8_t *ascii, int64_t len, int64_t *non_acgt, int64_t *region_bases)
{
    if (non_acgt) *non_acgt = 0;
    if (region_bases) *region_bases = len;
    if (!c || !c->has_regions) return len;
    int64_t m = 0, num_n = 0;
    for (size_t q = 0; q < c->regions.contig.size(); ++q) if (c->regions.contig[q] == contig_index) {
        m += c->regions.end[q] - c->regions.start[q];
        // the reference walks start..end INCLUSIVE with 1-based indexing (dwgsim.c:558-559); its read of
        // s[-1] for start == 0 is out of bounds there and is counted as non-ACGT here
        for (int64_t p = c->regions.start[q]; p <= (int64_t)c->regions.end[q]; ++p) { const int ch = (p >= 1 && p - 1 < len) ? ascii[p - 1] : 'N'; if (nt4(ch) >= 4) ++num_n; }
    }
    if (non_acgt) *non_acgt = num_n;
    if (region_bases) *region_bases = m;
    if (m == 0) return DWGSIM_HIP_SKIP_NO_REGION;
    if (0.95 < num_n / (double)m) return DWGSIM_HIP_SKIP_NON_ACGT;
    return m;
}

int dwgsim_hip_contig_set_placement_length(dwgsim_hip_ctx_t *c, int contig, int64_t l)
{
    int k = 0;
    Group *g = get_group(c, contig, &k);
    if (!g || l < 0) { if (c) c->err = "bad placement-length arguments"; return DWGSIM_HIP_ERR_ARG; }
    g->m[(size_t)k].l_place = l;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_set_mutation_input(dwgsim_hip_ctx_t *c, int type, const char *path, const char *const *names, const int64_t *lens, int n_contigs)
{
    if (!c || !path || type < 0 || type > 2 || n_contigs < 0 || (n_contigs && (!names || !lens))) { if (c) c->err = "bad mutation-input arguments"; return DWGSIM_HIP_ERR_ARG; }
    std::vector<ContigName> tab;
    for (int i = 0; i < n_contigs; ++i) tab.push_back(ContigName{names[i], lens[i]});
    std::string err;
    if (!parse_mutation_input(type, path, tab, c->mutin, err)) { c->err = err; c->has_mutin = false; return DWGSIM_HIP_ERR_ARG; }
    c->has_mutin = true;
    return DWGSIM_HIP_OK;
}

// mut_debug (mut.c:379-425): where the reference's asserts end the run (SIGABRT) the call returns DWGSIM_HIP_ERR_FAILED with the assert's text.
// The reference checks contig after contig, each before (mut.c:753) and after (:757) its justification: of the two verdicts of the group
// (smallest failing position of each pass) the one in the earlier contig -- the pre-justification one on a tie -- is the one it would have hit.
static int mut_debug_verdict(dwgsim_hip_ctx_t *c, const Group &g, uint64_t pre, uint64_t post)
{
    auto member_of = [&](uint64_t v) -> int { const int64_t p = (int64_t)(v >> 8); int k = 0; while (k + 1 < (int)g.m.size() && (int64_t)g.m[(size_t)k + 1].start <= p) ++k; return k; };
    uint64_t v = ~0ull;
    if (pre != ~0ull && post != ~0ull) v = member_of(post) < member_of(pre) ? post : pre;
    else v = pre != ~0ull ? pre : post;
    if (v == ~0ull) return DWGSIM_HIP_OK;
    static const char *what[4] = {"", "(c[0]&0x3) != (c[1]&0x3)", "(c[1]&0x3) != (c[2]&0x3)", "(c[0]&0x3) == (c[1]&0x3) || (c[0]&0x3) == (c[2]&0x3)"};
    const Member &m = g.m[(size_t)member_of(v)];
    char b[256]; snprintf(b, sizeof b, "dwgsim: src/mut.c: mut_debug: Assertion `%s' failed. [%s:%lld]\n", what[v & 3], m.name.c_str(), (long long)(v >> 8) - m.start + 1);
    c->err = b;
    return DWGSIM_HIP_ERR_FAILED;
}

// The insertion tables of haplotype h of a group: room for `entries` entries (+ 25 % + 64) and `bases` inserted bases (+ 25 % + 256; the
// allocation holds 16 bytes more: ins_bases_cap)
static int ensure_ins(dwgsim_hip_ctx_t *c, Group &g, int h, size_t entries, size_t bases)
{
    GroupMem &M = g.mem;
    const size_t want = sizeof(int32_t) * (entries + entries / 4 + 64);      // (int32 / uint32 entries alike)
    for (DevMem *b : {&M.d_ins_pos[h], &M.d_ins_len[h], &M.d_ins_off[h]}) HIPC(c, reserve(c, *b, sizeof(int32_t) * entries, want));
    HIPC(c, reserve(c, M.d_ins_bases[h], bases + 16, bases + bases / 4 + 256 + 16));
    return DWGSIM_HIP_OK;
}

// the read views and summaries of both haplotypes, made from every cell
static void make_views(hipStream_t st, const Group &g)
{
    const GroupMem &M = g.mem;
    launch_make_view(st, M.d_cells[0].get(), M.d_cells[1].get(), (int64_t)padded_cells(g) & ~(int64_t)15, g.total, M.d_view[0].get(), M.d_view[1].get(),
                     M.d_summ[0].get<uint16_t>(), M.d_summ[1].get<uint16_t>(), M.d_summ2[0].get<uint16_t>(), M.d_summ2[1].get<uint16_t>());
}

// dw_walk.hip k_dirty_chunks over the group's bitmap: restore = the chunks go back to the pristine copies, else their views and summaries are made again
static void dirty_chunks(hipStream_t st, bool restore, const Group &g)
{
    const GroupMem &M = g.mem;
    launch_dirty_chunks(st, restore, M.d_dirty.get<uint32_t>(), dirty_words(padded_cells(g)), g.total, M.d_ref.get(), M.d_refview.get(), M.d_refsumm.get<uint16_t>(), M.d_refsumm2.get<uint16_t>(),
                        M.d_cells[0].get(), M.d_cells[1].get(), M.d_view[0].get(), M.d_view[1].get(), M.d_summ[0].get<uint16_t>(), M.d_summ[1].get<uint16_t>(), M.d_summ2[0].get<uint16_t>(), M.d_summ2[1].get<uint16_t>());
}

// left-justification of the events of a walk: the cluster-parallel form or ("justify_seq", the cross-check) one thread for the whole group
static void justify(dwgsim_hip_ctx_t *c, hipStream_t st, const Event *ev, Count n, const ContigDev &cd)
{
    if (c->dbg.seq_justify) launch_justify_seq(st, ev, n, cd);
    else launch_justify(st, ev, n, cd, c->w_lo.get<int32_t>(), c->w_sufmin.get<int32_t>(), c->w_bound.get<uint8_t>());
}

// dwgsim_hip_debug_get("walk_form"): restore 0 none / 1 the dirty chunks / 2 whole buffers
static int64_t pack_walk_form(int attempt, bool file_driven, bool slots, int restore, bool dense)
{
    return (int64_t)attempt << 16 | (file_driven ? 1 : 0) << 12 | (slots ? 1 : 0) << 8 | restore << 4 | (dense ? 1 : 0);
}

// The walk of a group with file-driven mutations (-m / -b / -v, mut.c:644-745): the host resolved the entries (dwgsim_hip_mutate_async collected them), the
// GPU scatters them into the cells and left-justifies the indels; the views are made from every cell.  mut_debug runs before and after the justification.
static int walk_file_driven(dwgsim_hip_ctx_t *c, Group &g)
{
    hipStream_t st = c->walk_stream.get();
    const GroupMem &M = g.mem;
    WalkCounters *wc = c->d_wcounters.get<WalkCounters>();
    const uint32_t np = g.n_patch, nev = g.n_patch_ev;
    const size_t nev1 = nev ? nev : 1;
    if (np && (ensure(c, c->w_ppos, sizeof(int32_t) * np) || ensure(c, c->w_pcells, sizeof(uint16_t) * np) || ensure(c, c->w_ev, sizeof(Event) * nev1) ||
               ensure(c, c->w_lo, sizeof(int32_t) * nev1) || ensure(c, c->w_sufmin, sizeof(int32_t) * (nev1 + 64)) || ensure(c, c->w_bound, nev1))) return DWGSIM_HIP_ERR_DEVICE;      // (+ 64: segment minima of k_sufmin)
    c->dbg.walk_form = pack_walk_form(g.walk_attempt, true, false, g.walk_reset ? 2 : 0, true);
    HIPC(c, hipEventRecord(M.ev_walk0.get(), st));
    if (g.walk_reset) for (int h = 0; h < 2; ++h) if (const int rc = restore_pristine(c, g, h, R_CELLS, st)) return rc;
    HIPC(c, wc_fill(c, WC_FILE, 0xff, st));
    if (np) {
        HIPC(c, hipMemcpyAsync(c->w_ppos.get(), c->h_ppos.data(), sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
        HIPC(c, hipMemcpyAsync(c->w_pcells.get(), c->h_pcells.data(), sizeof(uint16_t) * np, hipMemcpyHostToDevice, st));
        if (nev) HIPC(c, hipMemcpyAsync(c->w_ev.get(), c->h_pev.data(), sizeof(Event) * nev, hipMemcpyHostToDevice, st));
        launch_apply_patches(st, c->w_ppos.get<int32_t>(), c->w_pcells.get<uint16_t>(), np, M.d_cells[0].get(), M.d_cells[1].get());
        launch_mut_debug(st, M.d_ref.get(), M.d_cells[0].get(), M.d_cells[1].get(), g.total, &wc->mut_debug[0]);      // mut.c:753
        if (nev) justify(c, st, c->w_ev.get<Event>(), Count{nullptr, nev}, group_dev(g));
        launch_mut_debug(st, M.d_ref.get(), M.d_cells[0].get(), M.d_cells[1].get(), g.total, &wc->mut_debug[1]);      // mut.c:757
    }
    make_views(st, g);
    g.dirty_all = true;
    HIPC(c, hipGetLastError());
    HIPC(c, wc_fetch(c, M, WC_FILE, st));
    HIPC(c, hipEventRecord(M.ev_walk.get(), st));
    return DWGSIM_HIP_OK;
}

// What one attempt of the random walk of a group takes, decided before anything is reserved or enqueued
enum class Restore { None, Chunks, All };
struct WalkPlan {
    uint32_t cap; size_t ncap, cap_bases;      // candidate capacity (ncap: what the buffers are sized for, at least 1); inserted-base pool per haplotype
    uint32_t nblk;                             // look-back words of k_site_scan_list (+ its ticket, + 1)
    bool use_slots; uint32_t nbs, slot_cap; size_t slot_bytes;      // the slot form of the site scan: blocks, entries per slot, bytes of all slots
    Restore restore;                           // what goes back to the pristine copies first
    bool dense;                                // views from every cell (the cross-check forms) / from the bitmap of dirty chunks
};

static WalkPlan walk_plan(const dwgsim_hip_ctx_t *c, const Group &g)
{
    WalkPlan P;
    P.cap = g.walk_cap; P.ncap = P.cap ? P.cap : 1; P.cap_bases = g.walk_cap_bases;
    P.nblk = (uint32_t)((g.total + SCAN_POS_PER_BLOCK - 1) / SCAN_POS_PER_BLOCK);
    // candidate sites -> ordered list.  First attempt: every block into a slot of its own, no block waits for another (dw_walk.hip k_site_scan_slots: mean +
    // 8 sigma + 32 entries per block of 65 536 positions); a re-run, a mutation rate at which the slots would be as large as the list itself, or
    // "site_slots" = 0: one kernel with a decoupled look-back
    P.nbs = site_scan_blocks(g.total);
    const double m = (double)site_scan_block_positions() * (c->prm.mut_rate > 0 ? c->prm.mut_rate : 0.0);
    P.slot_cap = (uint32_t)std::min<double>((double)site_scan_block_positions(), m + 8.0 * sqrt(m + 1.0) + 32.0);
    if (c->dbg.site_slot_cap >= 0) P.slot_cap = (uint32_t)std::max<int64_t>(1, c->dbg.site_slot_cap);
    P.slot_bytes = (size_t)P.nbs * P.slot_cap * sizeof(int32_t);
    P.use_slots = g.walk_attempt == 0 && c->dbg.site_slots != 0 && P.nbs > 0 && (c->dbg.site_slots > 0 || P.slot_bytes <= std::max<size_t>((size_t)64 << 20, P.ncap * 16));
    // where the group stands: fresh from the upload, or with the chunks the previous walk wrote -- those go back to the pristine copies --, or (a
    // capacity re-run, a walk that kept no bitmap) all of it
    P.restore = g.walk_attempt > 0 || g.dirty_all ? Restore::All : g.dirty_any ? Restore::Chunks : Restore::None;
    P.dense = c->dbg.seq_justify || c->dbg.dense_view;
    return P;
}

// room for the plan: the context's walk scratch and the group's insertion tables (at most one entry per candidate; the base pools are checked on the device)
static int walk_reserve(dwgsim_hip_ctx_t *c, Group &g, const WalkPlan &P)
{
    if (ensure(c, c->scratch_status, ((size_t)P.nblk + 2) * sizeof(uint64_t)) ||
        ensure(c, c->w_cand, sizeof(int32_t) * P.ncap) || ensure(c, c->w_ev, sizeof(Event) * P.ncap) ||
        ensure(c, c->w_flags, sizeof(uint4) * (P.ncap + 64)) ||      // (+ 64 rows / entries: the segment totals of k_scan4, the segment minima of k_sufmin)
        ensure(c, c->w_lo, sizeof(int32_t) * P.ncap) || ensure(c, c->w_sufmin, sizeof(int32_t) * (P.ncap + 64)) ||
        ensure(c, c->w_bound, P.ncap)) return DWGSIM_HIP_ERR_DEVICE;
    for (int h = 0; h < 2; ++h) if (const int rc = ensure_ins(c, g, h, P.ncap, P.cap_bases)) return rc;
    if (P.use_slots && (ensure(c, c->w_slots, P.slot_bytes) || ensure(c, c->w_slot_aux, 2 * (size_t)P.nbs * sizeof(uint32_t)))) return DWGSIM_HIP_ERR_DEVICE;
    return DWGSIM_HIP_OK;
}

// The kernels of the planned attempt: candidate sites, events, the cells, left-justification, the views of what was written
static int walk_launch(dwgsim_hip_ctx_t *c, Group &g, const WalkPlan &P)
{
    hipStream_t st = c->walk_stream.get();
    const WalkParams wp = walk_params(c);
    const SegTab seg = seg_tab(g);
    const GroupMem &M = g.mem;
    WalkCounters *wc = c->d_wcounters.get<WalkCounters>();
    int32_t *d_cand = c->w_cand.get<int32_t>(); Event *d_ev = c->w_ev.get<Event>(); uint4 *d_flags = c->w_flags.get<uint4>();
    uint32_t *tot4 = &wc->ins[0].entries;
    const Count nc{&wc->n_cand, P.cap};
    HIPC(c, wc_fill(c, WC_RANDOM, 0, st));
    // K1: candidate sites -> ordered list, from the pristine 4-bit view
    if (P.use_slots) launch_site_scan_slots(st, M.d_refview.get(), g.total, seg, wp, c->w_slots.get<int32_t>(), P.slot_cap, c->w_slot_aux.get<uint32_t>(), d_cand, P.cap, &wc->n_cand, &wc->slot_over);
    else {
        uint64_t *d_status = c->scratch_status.get<uint64_t>();      // the look-back words, and behind them the ticket
        HIPC(c, hipMemsetAsync(d_status, 0, ((size_t)P.nblk + 2) * sizeof(uint64_t), st));
        launch_site_scan_list(st, M.d_refview.get(), g.total, seg, wp, d_status, d_status + P.nblk, d_cand, P.cap, &wc->n_cand);
    }
    // K2: events, liveness, insertion-table allocation
    launch_events(st, d_cand, nc, M.d_ref.get(), seg, wp, d_ev, &wc->max_del);
    launch_resolve(st, d_ev, nc, &wc->max_del, d_flags, tot4);
    // K3 + K4
    ContigDev cd = group_dev(g);
    cd.tot4 = tot4; cd.cap_bases[0] = (uint32_t)std::min<size_t>(ins_bases_cap(g, 0), 0xFFFFFFFFu); cd.cap_bases[1] = (uint32_t)std::min<size_t>(ins_bases_cap(g, 1), 0xFFFFFFFFu);
    launch_apply(st, d_ev, nc, d_flags, cd, wp);
    // mut_debug (mut.c:753, :757) cannot fire on randomly drawn mutations and is not run here: a substitution always changes the base
    // ((c + 1..3) & 3, mut.c:621), a homozygous one writes the same cell to both haplotypes and a heterozygous one leaves the other
    // haplotype's cell as it was -- the reference base, also under a deletion or an insertion, before and after left-justification
    // (which only moves an indel over bases equal to its own).  File-driven mutations (-m / -b / -v, above) can violate all three.
    justify(c, st, d_ev, nc, cd);
    if (P.dense) {      // (the cross-check forms: the views are made from every cell as rounds 1-4 did)
        make_views(st, g);
        g.dirty_all = true;
    } else {
        // the chunks the walk may have written (every live event from the lower end of its justification scan to its last cell): their views and summaries
        launch_mark_dirty(st, d_ev, nc, c->w_lo.get<int32_t>(), M.d_dirty.get<uint32_t>());
        dirty_chunks(st, false, g);
        g.dirty_any = true;
    }
    HIPC(c, hipGetLastError());
    return DWGSIM_HIP_OK;
}

// One attempt of the random walk of a whole group, enqueued on the walk stream without any host read-back in between: buffers are sized for a
// capacity (candidate sites are a Binomial(l, mut_rate) draw: mean + 8 sigma), the kernels take their element counts from device memory, and
// the read-back at the end (dwgsim_hip_mutate_wait) also tells whether a capacity was exceeded -- then the walk is simply run again with
// exact sizes.  Everything is reserved before anything is enqueued: a failed allocation leaves the stream and the group as they were.
static int walk_random(dwgsim_hip_ctx_t *c, Group &g)
{
    const WalkPlan P = walk_plan(c, g);
    if (const int rc = walk_reserve(c, g, P)) return rc;
    c->dbg.walk_form = pack_walk_form(g.walk_attempt, false, P.use_slots, (int)P.restore, P.dense);
    hipStream_t st = c->walk_stream.get();
    HIPC(c, hipEventRecord(g.mem.ev_walk0.get(), st));
    if (P.restore == Restore::All) { for (int h = 0; h < 2; ++h) if (const int rc = restore_pristine(c, g, h, R_ALL, st)) return rc; }
    else if (P.restore == Restore::Chunks) dirty_chunks(st, true, g);
    if (P.restore != Restore::None) { if (const int rc = clear_dirty(c, g, st)) return rc; g.dirty_all = g.dirty_any = false; }
    if (const int rc = walk_launch(c, g, P)) return rc;
    HIPC(c, wc_fetch(c, g.mem, WC_RANDOM, st));
    HIPC(c, hipEventRecord(g.mem.ev_walk.get(), st));
    return DWGSIM_HIP_OK;
}

// File-driven mutations of a whole group in group coordinates: patched cells and indel events into the context's host lists, insertion payloads into hi
static void collect_file_mutations(dwgsim_hip_ctx_t *c, const Group &g, HostIns (&hi)[2])
{
    c->h_ppos.clear(); c->h_pcells.clear(); c->h_pev.clear();
    for (size_t k = 0; k < g.m.size(); ++k) {
        const Member &m = g.m[k];
        for (size_t q = 0; q < m.rc.pos.size(); ++q) {
            c->h_ppos.push_back(m.rc.pos[q] + m.start); c->h_pcells.push_back(m.rc.cells[q]);
            if (m.rc.cells[q] & 0x3030) { Event e; e.pos = m.rc.pos[q] + m.start; e.type = 4; e.hap = 3; e.base = 0; e.live = 1; e.len = 1; e.seg = (uint32_t)k; c->h_pev.push_back(e); }
        }
        for (int h = 0; h < 2; ++h) for (const InsPayload &ip : m.rc.ins[h]) {
            hi[h].pos.push_back(ip.pos + m.start); hi[h].len.push_back((uint32_t)ip.bases.size()); hi[h].off.push_back((uint32_t)hi[h].bases.size());
            hi[h].bases.insert(hi[h].bases.end(), ip.bases.begin(), ip.bases.end());
        }
    }
}

// the insertion tables the file's entries make, into the group's device tables
static int upload_ins_tables(dwgsim_hip_ctx_t *c, Group &g, HostIns (&hi)[2])
{
    for (int h = 0; h < 2; ++h) {
        const size_t n = hi[h].pos.size(), nb = hi[h].bases.size();
        g.n_ins[h] = (uint32_t)n; g.n_ins_bases[h] = (uint32_t)nb;
        if (const int rc = ensure_ins(c, g, h, n ? n : 1, nb ? nb : 1)) return rc;
        if (n) for (const InsTable &t : ins_tables(g.mem, h, hi[h])) HIPC(c, hipMemcpy(t.dev, t.host, t.bytes, hipMemcpyHostToDevice));
    }
    return DWGSIM_HIP_OK;
}

// The capacities the random walk of a group starts from: candidate sites are a Binomial(l, mut_rate) draw (mean + 8 sigma + 256), eight inserted bases per
// candidate + 4096 per haplotype.  dwgsim_hip_debug_option("walk_cap"): start too small, exercise the re-run.
static void initial_walk_caps(const dwgsim_hip_ctx_t *c, Group &g)
{
    double mean = 0;
    for (const Member &m : g.m) mean += (double)m.l * c->prm.mut_rate;
    g.walk_cap = (uint32_t)std::min<double>((double)g.total, mean + 8.0 * sqrt(mean + 1.0) + 256.0);
    g.walk_cap_bases = (size_t)g.walk_cap * 8 + 4096;
    if (c->dbg.walk_cap >= 0) { g.walk_cap = (uint32_t)c->dbg.walk_cap; g.walk_cap_bases = 1; }
}

int dwgsim_hip_mutate_async(dwgsim_hip_ctx_t *c, int contig)
{
    Group *gp = get_group(c, contig);
    if (!gp) return DWGSIM_HIP_ERR_ARG;
    Group &g = *gp;
    if (g.walk_pending) { c->err = "mutate: the group's previous walk was not waited for"; return DWGSIM_HIP_ERR_STATE; }
    // (walks of several groups may be in flight: they run one after the other on the walk stream and share its device scratch in stream order;
    // what the host reads back afterwards -- counts, mut_debug verdicts -- lands in the group's own page-locked mirror g.mem.h_wc)
    for (const Slot &sl : c->slot) if (sl.pending && sl.group == c->handles[(size_t)contig].group) { c->err = "mutate: a batch that reads this group is still in flight (wait for it first)"; return DWGSIM_HIP_ERR_STATE; }
    HIPC(c, hipSetDevice(c->device));
    g.walk_reset = g.mutated;      // walked before: the cells start again from the resident packed reference
    for (int h = 0; h < 2; ++h) g.n_ins[h] = g.n_ins_bases[h] = 0;
    g.mutated = true; g.n_cand = 0; g.list_valid = false; g.depth_valid = false;
    for (int h = 0; h < 2; ++h) g.hap_text[h].valid = g.hap_chain[h].valid = false;
    g.walk_attempt = 0;
    if (g.total == 0) return DWGSIM_HIP_OK;
    if (c->has_mutin) {
        HIPC(c, hipStreamSynchronize(c->walk_stream.get()));      // (an earlier group's walk may still be copying from the host lists)
        HostIns hi[2];
        collect_file_mutations(c, g, hi);
        g.n_patch = (uint32_t)c->h_ppos.size(); g.n_patch_ev = (uint32_t)c->h_pev.size();
        g.n_cand = g.n_patch_ev;
        HIPC(c, hipStreamSynchronize(c->walk_stream.get()));      // (the tables are copied from short-lived host vectors)
        if (const int rc = upload_ins_tables(c, g, hi)) return rc;
    } else initial_walk_caps(c, g);
    if (const int rc = c->has_mutin ? walk_file_driven(c, g) : walk_random(c, g)) return rc;
    g.walk_pending = true;
    return DWGSIM_HIP_OK;
}

// Does the attempt the counters come from fit its capacities?  (A block of the site scan that outgrew its slot: nothing behind it ran, the candidate count was set to 0.)
static bool walk_fits(const WalkCounters &w, const Group &g)
{
    return !w.slot_over && w.n_cand <= g.walk_cap && w.ins[0].bases <= ins_bases_cap(g, 0) && w.ins[1].bases <= ins_bases_cap(g, 1);
}

// The capacities of the exact re-run (the counts read back are those of the complete candidate list unless it was truncated: generous ones then)
static void exact_walk_caps(const WalkCounters &w, Group &g)
{
    g.walk_cap = (uint32_t)std::min<uint64_t>((uint64_t)g.total, (w.slot_over ? (uint64_t)w.n_cand_true : w.n_cand) + 16);
    g.walk_cap_bases = std::max<size_t>(g.walk_cap_bases, (size_t)std::max(w.ins[0].bases, w.ins[1].bases) * 2 + (size_t)g.walk_cap * 8 + 4096);
}

int dwgsim_hip_mutate_wait(dwgsim_hip_ctx_t *c, int contig)
{
    Group *gp = get_group(c, contig);
    if (!gp) return DWGSIM_HIP_ERR_ARG;
    Group &g = *gp;
    if (!g.walk_pending) return g.mutated ? DWGSIM_HIP_OK : (c->err = "mutate_wait: no walk was enqueued for this group", DWGSIM_HIP_ERR_STATE);
    HIPC(c, hipSetDevice(c->device));
    const WalkCounters &w = *g.mem.h_wc.get<WalkCounters>();
    for (;;) {      // wait, verdict, grow, enqueue again
        HIPC(c, hipEventSynchronize(g.mem.ev_walk.get()));
        { float ms = 0; if (hipEventElapsedTime(&ms, g.mem.ev_walk0.get(), g.mem.ev_walk.get()) == hipSuccess) c->dbg.walk_us += 1e3 * ms; else (void)hipGetLastError(); }      // (analysis: dwgsim_hip_debug_get "walk_us")
        if (c->has_mutin) {
            g.walk_pending = false;
            return g.n_patch ? mut_debug_verdict(c, g, w.mut_debug[0], w.mut_debug[1]) : DWGSIM_HIP_OK;
        }
        const bool fits = walk_fits(w, g);
        if (fits || g.walk_attempt >= 2) {
            g.walk_pending = false;
            if (!fits) { c->err = "mutation walk: capacities still exceeded after an exact re-run"; return DWGSIM_HIP_ERR_FAILED; }
            g.n_cand = (uint32_t)w.n_cand;
            for (int h = 0; h < 2; ++h) { g.n_ins[h] = w.ins[h].entries; g.n_ins_bases[h] = w.ins[h].bases; }
            return DWGSIM_HIP_OK;
        }
        exact_walk_caps(w, g);
        ++g.walk_attempt;
        if (const int rc = walk_random(c, g)) { g.walk_pending = false; return rc; }
    }
}

int dwgsim_hip_mutate_poll(dwgsim_hip_ctx_t *c, int contig)
{
    Group *gp = get_group(c, contig);
    if (!gp) return DWGSIM_HIP_ERR_ARG;
    if (!gp->walk_pending) return 1;
    HIPC(c, hipSetDevice(c->device));
    const hipError_t e = hipEventQuery(gp->mem.ev_walk.get());
    if (e == hipSuccess) return 1;
    (void)hipGetLastError();
    return e == hipErrorNotReady ? 0 : (c->err = "mutate_poll: device error", DWGSIM_HIP_ERR_DEVICE);
}

int dwgsim_hip_mutate_contig(dwgsim_hip_ctx_t *c, int contig)
{
    const int rc = dwgsim_hip_mutate_async(c, contig);
    if (rc != DWGSIM_HIP_OK) return rc;
    return dwgsim_hip_mutate_wait(c, contig);
}

// ---- mutations.txt / mutations.vcf from the sparse list of mutated cells (mut.c:781-893) ----
namespace {
// The text is made by plain appends (a vsnprintf per field cost 0.2 us per mutation: 50 ms for a 250 Mb chromosome, during which the worker of
// round 4's job level enqueued nothing); it is also a pure function of the list, so that it can be made by another thread than the one that
// drives the device (dwgsim_hip_mutations_take / dwgsim_hip_mutlist_text).
struct TextOut {
    std::string &s;
    void ch(char c) { s.push_back(c); }
    void str(const char *p, size_t n) { s.append(p, n); }
    void lit(const char *p) { s.append(p); }
    void num(long long v)
    {
        char b[24]; int n = 0; unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        do { b[n++] = (char)('0' + u % 10); u /= 10; } while (u);
        if (v < 0) s.push_back('-');
        while (n) s.push_back(b[--n]);
    }
};
struct ListView {      // the mutated cells of a group (group coordinates) and its insertion tables
    const int32_t *pos; const uint32_t *cells; size_t n; const HostIns *ins;
};
void ins_text(const HostIns &t, int32_t pos, std::string &tmp)
{
    tmp.clear();
    auto it = std::lower_bound(t.pos.begin(), t.pos.end(), pos);
    if (it == t.pos.end() || *it != pos) return;
    const size_t k = (size_t)(it - t.pos.begin());
    for (uint32_t q = 0; q < t.len[k]; ++q) tmp.push_back("ACGTN"[t.bases[t.off[k] + q] & 3]);
}
// mut_print (mut.c:781-893) for one contig: name, first cell s0 and length l in the group's coordinates
// With tvcf_s the records of the truth VCF are made beside those of the VCF: the same line with FORMAT and one sample column behind it, GT:AD:DP from
// depth = the counters of this contig's slice of the list, two per cell (the rule: dw_truth.hpp k_truth_depth).  GT is the phase pl says; AD is ref,alt -- alt
// the ends of the haplotype(s) that carry the record's allele, ref those of the other haplotype where its cell is unmutated (else 0; none when pl = 3) --
// and DP both counters.  A deletion's record takes the counters of the first deleted cell of the run.
void format_mutations(const ListView &g, const std::string &name, int64_t s0, int64_t l, std::string &txt_s, std::string &vcf_s, const uint64_t *depth = nullptr, std::string *tvcf_s = nullptr)
{
    txt_s.clear(); vcf_s.clear();
    if (tvcf_s) tvcf_s->clear();
    // this contig's slice of the list, positions inside the contig
    const size_t e0 = (size_t)(std::lower_bound(g.pos, g.pos + g.n, (int32_t)s0) - g.pos);
    const size_t e1 = (size_t)(std::lower_bound(g.pos, g.pos + g.n, (int32_t)(s0 + l)) - g.pos);
    txt_s.reserve((e1 - e0) * (name.size() + 20)); vcf_s.reserve((e1 - e0) * (name.size() + 56));
    // sparse restatement of the per-position loop: only listed positions can print; "previous position
    // mutated" (mut_prev, mut.c:890-891) is "position i-1 is listed with a mutated cell on that haplotype"
    static const char B5[] = "ACGTN";       // B5[5] is the terminating NUL, as in the reference for code 5 ('-')
    TextOut txt{txt_s}, vcf{vcf_s};
    // (a %c of the NUL of B5[5] prints a NUL byte in the reference; r0 < 4 and substituted / inserted bases are 0-3 here, deleted reference bases too)
    std::string tmp;
    auto cell = [&](size_t e, int h) -> uint8_t { return (uint8_t)(h ? g.cells[e] >> 8 : g.cells[e]); };
    auto refc = [&](size_t e) -> uint8_t { return (uint8_t)(g.cells[e] >> 16); };          // nst_nt4_table code of the reference base
    auto prevc = [&](size_t e) -> uint8_t { return (uint8_t)(g.cells[e] >> 24); };         // ... of the base in front of it
    size_t rec_at = 0;      // where the VCF record being made starts
    auto vcf_head = [&](long long at) { rec_at = vcf_s.size(); vcf.str(name.data(), name.size()); vcf.ch('\t'); vcf.num(at); vcf.lit("\t.\t"); };
    auto sample = [&](size_t e, int pl) {      // the finished record of cell e once more, with its sample column
        if (!tvcf_s) return;
        TextOut t{*tvcf_s};
        t.str(vcf_s.data() + rec_at, vcf_s.size() - rec_at - 1);
        const uint64_t n1 = depth ? depth[2 * (e - e0)] : 0, n2 = depth ? depth[2 * (e - e0) + 1] : 0;      // (no counters: nothing was simulated)
        const uint64_t alt = pl == 3 ? n1 + n2 : pl == 1 ? n1 : n2;
        const uint64_t ref = pl == 3 ? 0 : (cell(e, pl == 1 ? 1 : 0) & TMASK) == T_NONE ? (pl == 1 ? n2 : n1) : 0;
        t.lit("\tGT:AD:DP\t"); t.lit(pl == 3 ? "1|1" : pl == 1 ? "1|0" : "0|1");
        t.ch(':'); t.num((long long)ref); t.ch(','); t.num((long long)alt); t.ch(':'); t.num((long long)(n1 + n2)); t.ch('\n');
    };
    for (size_t e = e0; e < e1; ++e) {
        const int64_t i = g.pos[e] - s0;
        const uint8_t r0 = refc(e), c1 = cell(e, 0), c2 = cell(e, 1);
        if (r0 >= 4) continue;
        const bool adj = e > e0 && g.pos[e - 1] == g.pos[e] - 1;
        const bool prev0 = adj && (cell(e - 1, 0) & TMASK) != T_NONE, prev1 = adj && (cell(e - 1, 1) & TMASK) != T_NONE;
        txt.str(name.data(), name.size()); txt.ch('\t'); txt.num((long long)i + 1); txt.ch('\t');
        const bool hom = (c1 & BTMASK) == (c2 & BTMASK);
        const uint8_t t1 = c1 & TMASK, t2 = c2 & TMASK;
        if (hom ? t1 == T_SUB : (t1 == T_SUB || t2 == T_SUB)) {
            if (hom) {
                txt.ch(B5[r0]); txt.ch('\t'); txt.ch(B5[c1 & 0xf]); txt.lit("\t3\n");
                vcf_head((long long)i + 1); vcf.ch(B5[r0]); vcf.ch('\t'); vcf.ch(B5[c1 & 0xf]); vcf.lit("\t100\tPASS\tAF=1.0;pl=3;mt=SUBSTITUTE\n");
                sample(e, 3);
            } else {
                const int hap = t1 == T_SUB ? 1 : 2;
                txt.ch(B5[r0]); txt.ch('\t'); txt.ch("XACMGRSVTWYHKDBN"[1 << (c1 & 3) | 1 << (c2 & 3)]); txt.ch('\t'); txt.ch((char)('0' + hap)); txt.ch('\n');
                vcf_head((long long)i + 1); vcf.ch(B5[r0]); vcf.ch('\t'); vcf.ch(B5[(hap == 1 ? c1 : c2) & 0xf]); vcf.lit("\t100\tPASS\tAF=0.5;pl="); vcf.ch((char)('0' + hap)); vcf.lit(";mt=SUBSTITUTE\n");
                sample(e, hap);
            }
        } else if (hom ? t1 == T_DEL : (t1 == T_DEL || t2 == T_DEL)) {
            const int pl = hom ? 3 : (t1 == T_DEL ? 1 : 2);
            txt.ch(B5[r0]); txt.lit("\t-\t"); txt.ch((char)('0' + pl)); txt.ch('\n');
            const bool open = hom ? (!prev0 || !prev1) : !(pl == 1 ? prev0 : prev1);
            if (open) {      // one VCF record for the run, anchored at the previous reference base (mut.c:801-815)
                vcf_head((long long)i);
                if (i > 0) vcf.ch(B5[prevc(e)]);
                size_t ee = e; int64_t j = i;
                for (;;) {
                    vcf.ch(B5[refc(ee)]);
                    if (j + 1 >= l) break;
                    // cell at j+1: listed -> its cells, else unmutated
                    if (ee + 1 < e1 && g.pos[ee + 1] - s0 == j + 1) {
                        ++ee; ++j;
                        const uint8_t a1 = cell(ee, 0), a2 = cell(ee, 1);
                        const bool h2 = (a1 & BTMASK) == (a2 & BTMASK);
                        if (!(h2 == hom && ((pl == 2 ? a2 : a1) & TMASK) == T_DEL)) break;
                    } else break;
                }
                if (i > 0) { vcf.ch('\t'); vcf.ch(B5[prevc(e)]); } else vcf.lit("\t.");
                vcf.lit("\t100\tPASS\tAF="); vcf.lit(hom ? "1.0" : "0.5"); vcf.lit(";pl="); vcf.ch((char)('0' + pl)); vcf.lit(";mt=DELETE\n");
                sample(e, pl);
            }
        } else {
            const int pl = hom ? 3 : (t1 == T_INS ? 1 : 2);
            ins_text(g.ins[pl == 2 ? 1 : 0], g.pos[e], tmp);
            txt.lit("-\t"); txt.str(tmp.data(), tmp.size()); txt.ch('\t'); txt.ch((char)('0' + pl)); txt.ch('\n');
            vcf_head((long long)i + 1); vcf.ch(B5[r0]); vcf.ch('\t'); vcf.ch(B5[r0]); vcf.str(tmp.data(), tmp.size());
            vcf.lit("\t100\tPASS\tAF="); vcf.lit(hom ? "1.0" : "0.5"); vcf.lit(";pl="); vcf.ch((char)('0' + pl)); vcf.lit(";mt=INSERT\n");
            sample(e, pl);
        }
    }
}

// The positions of a walked group's mutated cells (group coordinates, ascending) into the context's l_pos, on the walk stream: *n_out of them, known here
// (the call waits for the count), the positions themselves enqueued behind it
int collect_listed_positions(dwgsim_hip_ctx_t *c, Group &g, uint32_t *n_out)
{
    *n_out = 0;
    if (g.total <= 0 || g.n_cand == 0) return DWGSIM_HIP_OK;
    hipStream_t st = c->walk_stream.get();
    const uint32_t nblk = (uint32_t)((g.total + SCAN_POS_PER_BLOCK - 1) / SCAN_POS_PER_BLOCK);
    if (ensure(c, c->scratch_mask, (size_t)nblk * SCAN_THREADS * sizeof(uint16_t))) return DWGSIM_HIP_ERR_DEVICE;
    if (ensure(c, c->scratch_cnt, (size_t)nblk * sizeof(uint32_t))) return DWGSIM_HIP_ERR_DEVICE;
    uint16_t *d_mask = c->scratch_mask.get<uint16_t>(); uint32_t *d_cnt = c->scratch_cnt.get<uint32_t>();
    launch_collect_mask(st, g.mem.d_cells[0].get(), g.mem.d_cells[1].get(), g.total, d_mask, d_cnt);
    launch_scan_excl(st, d_cnt, nblk, &c->d_wcounters.get<WalkCounters>()->n_listed);
    HIPC(c, wc_fetch(c, g.mem, WC_LISTED, st));
    HIPC(c, hipStreamSynchronize(st));
    const uint32_t n = (uint32_t)g.mem.h_wc.get<WalkCounters>()->n_listed;
    if (n) {
        if (ensure(c, c->l_pos, sizeof(int32_t) * (size_t)n)) return DWGSIM_HIP_ERR_DEVICE;
        launch_compact(st, d_mask, d_cnt, c->l_pos.get<int32_t>(), g.total, n);
    }
    *n_out = n;
    return DWGSIM_HIP_OK;
}

// the mutated cells of a walked group (positions in group coordinates, cells + reference codes) and its insertion tables, fetched once
int fetch_mutated_list(dwgsim_hip_ctx_t *c, Group &g)
{
    if (g.list_valid) return DWGSIM_HIP_OK;
    g.pos.clear(); g.cells.clear();
    for (int h = 0; h < 2; ++h) g.ins[h] = HostIns();
    hipStream_t st = c->walk_stream.get();
    if (g.total > 0 && g.n_cand > 0) {
        uint32_t n = 0;
        if (const int rc = collect_listed_positions(c, g, &n)) return rc;
        if (n) {
            if (ensure(c, c->l_cells, sizeof(uint32_t) * (size_t)n)) return DWGSIM_HIP_ERR_DEVICE;
            launch_gather(st, c->l_pos.get<int32_t>(), n, g.mem.d_ref.get(), g.mem.d_cells[0].get(), g.mem.d_cells[1].get(), c->l_cells.get<uint32_t>());
            g.pos.resize(n); g.cells.resize(n);
            HIPC(c, hipMemcpyAsync(g.pos.data(), c->l_pos.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
            HIPC(c, hipMemcpyAsync(g.cells.data(), c->l_cells.get(), sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        }
        for (int h = 0; h < 2; ++h) if (g.n_ins[h]) {
            g.ins[h].pos.resize(g.n_ins[h]); g.ins[h].len.resize(g.n_ins[h]); g.ins[h].off.resize(g.n_ins[h]); g.ins[h].bases.resize(g.n_ins_bases[h]);
            for (const InsTable &t : ins_tables(g.mem, h, g.ins[h])) HIPC(c, hipMemcpyAsync(t.host, t.dev, t.bytes, hipMemcpyDeviceToHost, st));
        }
        HIPC(c, hipStreamSynchronize(st));
    }
    g.list_valid = true;
    return DWGSIM_HIP_OK;
}

// The true read depth (dwgsim_hip_set_truth_depth): the group's own copy of its listed positions and the zeroed counters behind them, made before the group's
// first batch with the feature on.  The call returns when both are in place (the batches run on another stream).
int depth_prepare(dwgsim_hip_ctx_t *c, Group &g)
{
    if (g.depth_valid) return DWGSIM_HIP_OK;
    uint32_t n = 0;
    if (const int rc = collect_listed_positions(c, g, &n)) return rc;
    g.depth_pos.assign(n, 0);
    if (n) {
        hipStream_t st = c->walk_stream.get();
        HIPC(c, reserve(c, g.mem.d_depth_pos, sizeof(int32_t) * (size_t)n, sizeof(int32_t) * ((size_t)n + n / 8 + 1024)));
        HIPC(c, reserve(c, g.mem.d_depth_cnt, 2 * sizeof(uint64_t) * (size_t)n, 2 * sizeof(uint64_t) * ((size_t)n + n / 8 + 1024)));
        HIPC(c, hipMemcpyAsync(g.mem.d_depth_pos.get(), c->l_pos.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
        HIPC(c, hipMemsetAsync(g.mem.d_depth_cnt.get(), 0, 2 * sizeof(uint64_t) * (size_t)n, st));
        HIPC(c, hipMemcpyAsync(g.depth_pos.data(), c->l_pos.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPC(c, hipStreamSynchronize(st));
    }
    g.depth_valid = true;
    return DWGSIM_HIP_OK;
}
} // namespace

int dwgsim_hip_mutations_text(dwgsim_hip_ctx_t *c, int contig, const char **txt, size_t *txt_len, const char **vcf, size_t *vcf_len)
{
    int km = 0;
    Group *gp = get_group(c, contig, &km);
    if (!gp) return DWGSIM_HIP_ERR_ARG;
    Group &g = *gp;
    if (!g.mutated || g.walk_pending) { c->err = "mutate_contig must run first"; return DWGSIM_HIP_ERR_STATE; }
    HIPC(c, hipSetDevice(c->device));
    if (const int rc = fetch_mutated_list(c, g)) return rc;
    const Member &m = g.m[(size_t)km];
    format_mutations(ListView{g.pos.data(), g.cells.data(), g.pos.size(), g.ins}, m.name, m.start, m.l, c->txt, c->vcf);
    if (txt) *txt = c->txt.data();
    if (txt_len) *txt_len = c->txt.size();
    if (vcf) *vcf = c->vcf.data();
    if (vcf_len) *vcf_len = c->vcf.size();
    return DWGSIM_HIP_OK;
}

// The same in two halves, for callers that keep the device busy meanwhile (the job level): `take` fetches the group's list of mutated cells (device
// work, on the calling thread) and hands it over as an object of its own; `mutlist_text` makes the text of one of the group's contigs from it --
// no context, no device: any thread may call it while the context goes on with the group's reads.
struct dwgsim_hip_mutlist {
    std::vector<int32_t> pos; std::vector<uint32_t> cells; HostIns ins[2];
    struct M { std::string name; int64_t l; int32_t start; };
    std::vector<M> m;
    std::string txt, vcf, tvcf;
};

dwgsim_hip_mutlist_t *dwgsim_hip_mutations_take(dwgsim_hip_ctx_t *c, int contig, int *n_contigs)
{
    if (n_contigs) *n_contigs = 0;
    if (!c) return nullptr;
    Group *gp = get_group(c, contig);
    if (!gp) return nullptr;
    Group &g = *gp;
    if (!g.mutated || g.walk_pending) { c->err = "mutate_contig must run first"; return nullptr; }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "mutations_take: device error"; return nullptr; }
    if (fetch_mutated_list(c, g)) return nullptr;
    auto *L = new dwgsim_hip_mutlist();
    L->pos.swap(g.pos); L->cells.swap(g.cells);
    for (int h = 0; h < 2; ++h) { L->ins[h] = std::move(g.ins[h]); g.ins[h] = HostIns(); }
    g.list_valid = false;      // (a later mutations_text for this group fetches it again)
    for (const Member &m : g.m) L->m.push_back({m.name, m.l, m.start});
    if (n_contigs) *n_contigs = (int)L->m.size();
    return L;
}

int dwgsim_hip_mutlist_text(dwgsim_hip_mutlist_t *L, int k, const char **txt, size_t *txt_len, const char **vcf, size_t *vcf_len)
{
    if (!L || k < 0 || k >= (int)L->m.size()) return DWGSIM_HIP_ERR_ARG;
    const auto &m = L->m[(size_t)k];
    format_mutations(ListView{L->pos.data(), L->cells.data(), L->pos.size(), L->ins}, m.name, m.start, m.l, L->txt, L->vcf);
    if (txt) *txt = L->txt.data();
    if (txt_len) *txt_len = L->txt.size();
    if (vcf) *vcf = L->vcf.data();
    if (vcf_len) *vcf_len = L->vcf.size();
    return DWGSIM_HIP_OK;
}

// ... and the records of the truth VCF (DESIGN.md "6f") of contig k from the counters the caller passes: the contig's slice of the list, two per cell, as
// dwgsim_hip_truth_depth_fetch gives them -- or the sum of what several contexts gave
int dwgsim_hip_mutlist_truth_vcf_text(dwgsim_hip_mutlist_t *L, int k, const uint64_t *counts, size_t n_cells, const char **vcf, size_t *vcf_len)
{
    if (!L || k < 0 || k >= (int)L->m.size() || (!counts && n_cells)) return DWGSIM_HIP_ERR_ARG;
    const auto &m = L->m[(size_t)k];
    const int32_t *p0 = L->pos.data(), *p1 = p0 + L->pos.size();
    if (counts && (size_t)(std::lower_bound(p0, p1, (int32_t)(m.start + m.l)) - std::lower_bound(p0, p1, m.start)) != n_cells) return DWGSIM_HIP_ERR_ARG;      // (not this contig's counters)
    format_mutations(ListView{L->pos.data(), L->cells.data(), L->pos.size(), L->ins}, m.name, m.start, m.l, L->txt, L->vcf, counts, &L->tvcf);
    if (vcf) *vcf = L->tvcf.data();
    if (vcf_len) *vcf_len = L->tvcf.size();
    return DWGSIM_HIP_OK;
}

void dwgsim_hip_mutlist_free(dwgsim_hip_mutlist_t *L) { delete L; }

// ---- the two finished haplotypes as FASTA text (dw_walk.hip k_hap_len / k_hap_headers / k_hap_write) ----
// On the walk stream, behind the group's walk: emitted bases per block of cells, their scan, the records placed by the host from the prefix at every
// contig's first block, then the text.  The call returns when the text is complete (what it enqueues is two passes over the cells).
int dwgsim_hip_haplotype_fasta(dwgsim_hip_ctx_t *c, int contig, int hap, int width, uint64_t *bytes)
{
    Group *gp = get_group(c, contig);
    if (!gp) return DWGSIM_HIP_ERR_ARG;
    Group &g = *gp;
    if (hap < 0 || hap > 1 || width < 0) { c->err = "haplotype_fasta: hap must be 0 or 1 and width >= 0"; return DWGSIM_HIP_ERR_ARG; }
    if (!g.mutated || g.walk_pending) { c->err = "mutate_contig must run first"; return DWGSIM_HIP_ERR_STATE; }
    const int gid = (int)(gp - c->groups.data());
    Group::HapText &T = g.hap_text[hap];
    if (!(T.valid && T.width == width)) {
        HIPC(c, hipSetDevice(c->device));
        T.valid = false;
        // (the scan of the blocks is a 32-bit one: cells and inserted bases of a group stay below 2^32 together; the TEXT offsets are 64-bit)
        if ((uint64_t)g.total + g.n_ins_bases[hap] > 0xFFFFFFFFull) { c->err = "haplotype_fasta: more than 2^32 bases in one group"; return DWGSIM_HIP_ERR_UNSUP; }
        GroupMem &M = g.mem;
        hipStream_t st = c->walk_stream.get();
        const size_t n = g.m.size();
        const uint32_t nblk = (uint32_t)((g.total + SCAN_POS_PER_BLOCK - 1) / SCAN_POS_PER_BLOCK);
        if (ensure(c, c->scratch_cnt, ((size_t)nblk + 1) * sizeof(uint32_t))) return DWGSIM_HIP_ERR_DEVICE;
        uint32_t *d_cnt = c->scratch_cnt.get<uint32_t>();
        HapDev hd[2]; fill_haps(g, hd);
        const SegTab seg = seg_tab(g);
        std::vector<uint32_t> pre((size_t)nblk + 1, 0);      // emitted bases in front of every block, and (the last entry) of the group
        for (DevEvent &e : c->hap_ev) HIPC(c, e.create());
        if (nblk) {
            HIPC(c, hipMemsetAsync(d_cnt + nblk, 0, sizeof(uint32_t), st));
            HIPC(c, hipEventRecord(c->hap_ev[0].get(), st));
            launch_hap_len(st, hd[hap], seg, g.total, d_cnt);
            launch_scan_excl(st, d_cnt, nblk + 1, nullptr);
            HIPC(c, hipEventRecord(c->hap_ev[1].get(), st));
            HIPC(c, hipMemcpyAsync(pre.data(), d_cnt, ((size_t)nblk + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPC(c, hipStreamSynchronize(st));
        }
        std::vector<HapRec> rec(n); std::vector<uint8_t> pool;
        T.off.assign(n, 0); T.len.assign(n, 0); T.bases.assign(n, 0);
        uint64_t at = 0;
        for (size_t k = 0; k < n; ++k) {
            const Member &m = g.m[k];
            const size_t b0 = (size_t)(m.start / SCAN_POS_PER_BLOCK), b1 = m.l > 0 ? (size_t)((m.start + m.l + SCAN_POS_PER_BLOCK - 1) / SCAN_POS_PER_BLOCK) : b0;
            HapRec &R = rec[k];
            R.rec_off = at; R.hdr_off = (uint32_t)pool.size(); R.hdr_len = (uint32_t)m.name.size() + 2; R.base0 = pre[b0]; R.n_bases = pre[b1] - pre[b0]; R.pad_ = 0;
            pool.push_back('>'); pool.insert(pool.end(), m.name.begin(), m.name.end()); pool.push_back('\n');
            const uint64_t body = R.n_bases ? (uint64_t)R.n_bases + (width ? ((uint64_t)R.n_bases + (uint64_t)width - 1) / (uint64_t)width : 1u) : 0u;
            T.off[k] = at; T.len[k] = R.hdr_len + body; T.bases[k] = R.n_bases;
            at += T.len[k];
        }
        if (ensure(c, M.d_hap_text[hap], (size_t)at + 64) || ensure(c, M.d_hap_rec, sizeof(HapRec) * n) || ensure(c, M.d_hap_pool, pool.size())) return DWGSIM_HIP_ERR_DEVICE;
        HIPC(c, hipMemcpyAsync(M.d_hap_rec.get(), rec.data(), sizeof(HapRec) * n, hipMemcpyHostToDevice, st));
        HIPC(c, hipMemcpyAsync(M.d_hap_pool.get(), pool.data(), pool.size(), hipMemcpyHostToDevice, st));
        HIPC(c, hipEventRecord(c->hap_ev[2].get(), st));
        launch_hap_write(st, hd[hap], seg, g.total, d_cnt, M.d_hap_rec.get<HapRec>(), (uint32_t)n, M.d_hap_pool.get(), (uint32_t)width, M.d_hap_text[hap].get());
        HIPC(c, hipEventRecord(c->hap_ev[3].get(), st));
        HIPC(c, hipGetLastError());
        DevMem yard;      // "hap_yardstick" (measurement only): a device-to-device copy of as many bytes as the text, behind it on the same stream (the second of two is timed)
        if (c->dbg.hap_yardstick && at) {
            HIPC(c, reserve(c, yard, (size_t)at, (size_t)at));
            HIPC(c, hipMemcpyAsync(yard.get(), M.d_hap_text[hap].get(), (size_t)at, hipMemcpyDeviceToDevice, st));
            HIPC(c, hipEventRecord(c->hap_ev[4].get(), st));
            HIPC(c, hipMemcpyAsync(yard.get(), M.d_hap_text[hap].get(), (size_t)at, hipMemcpyDeviceToDevice, st));
            HIPC(c, hipEventRecord(c->hap_ev[5].get(), st));
        }
        HIPC(c, hipStreamSynchronize(st));      // (the records and header lines go up from vectors of this call)
        {   // (analysis: dwgsim_hip_debug_get "hap_len_us" / "hap_write_us" / "hap_copy_us", of the text built last)
            float ms = 0;
            c->dbg.hap_len_us = nblk && hipEventElapsedTime(&ms, c->hap_ev[0].get(), c->hap_ev[1].get()) == hipSuccess ? 1e3 * ms : 0;
            c->dbg.hap_write_us = hipEventElapsedTime(&ms, c->hap_ev[2].get(), c->hap_ev[3].get()) == hipSuccess ? 1e3 * ms : 0;
            c->dbg.hap_copy_us = yard && hipEventElapsedTime(&ms, c->hap_ev[4].get(), c->hap_ev[5].get()) == hipSuccess ? 1e3 * ms : 0;
            (void)hipGetLastError();
        }
        T.width = width; T.bytes = at; T.valid = true;
    }
    c->hap_cur[hap] = gid;
    if (bytes) *bytes = T.bytes;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_haplotype_layout(dwgsim_hip_ctx_t *c, int contig, int hap, uint64_t *offset, uint64_t *bytes, int64_t *bases)
{
    int km = 0;
    Group *gp = get_group(c, contig, &km);
    if (!gp) return DWGSIM_HIP_ERR_ARG;
    if (hap < 0 || hap > 1) { c->err = "haplotype_layout: hap must be 0 or 1"; return DWGSIM_HIP_ERR_ARG; }
    const Group::HapText &T = gp->hap_text[hap];
    if (!T.valid) { c->err = "haplotype_layout: dwgsim_hip_haplotype_fasta must run first"; return DWGSIM_HIP_ERR_STATE; }
    if (offset) *offset = T.off[(size_t)km];
    if (bytes) *bytes = T.len[(size_t)km];
    if (bases) *bases = T.bases[(size_t)km];
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_haplotype_fetch(dwgsim_hip_ctx_t *c, int hap, uint64_t offset, void *host_dst, size_t n)
{
    if (!c) return DWGSIM_HIP_ERR_ARG;
    if (hap < 0 || hap > 1 || (!host_dst && n)) { c->err = "bad haplotype_fetch arguments"; return DWGSIM_HIP_ERR_ARG; }
    const int gid = c->hap_cur[hap];
    if (gid < 0 || !c->groups[(size_t)gid].alive || !c->groups[(size_t)gid].hap_text[hap].valid) { c->err = "haplotype_fetch: dwgsim_hip_haplotype_fasta must run first"; return DWGSIM_HIP_ERR_STATE; }
    const Group &g = c->groups[(size_t)gid];
    const uint64_t total = g.hap_text[hap].bytes;
    if (offset > total || (uint64_t)n > total - offset) { c->err = "haplotype_fetch: past the end of the text"; return DWGSIM_HIP_ERR_ARG; }
    if (n == 0) return DWGSIM_HIP_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, c->hap_stream.create());
    const uint8_t *src = g.mem.d_hap_text[hap].get<uint8_t>() + offset;
    if (is_page_locked(host_dst)) {
        HIPC(c, hipMemcpyAsync(host_dst, src, n, hipMemcpyDeviceToHost, c->hap_stream.get()));
        HIPC(c, hipStreamSynchronize(c->hap_stream.get()));
        return DWGSIM_HIP_OK;
    }
    // double-buffered page-locked staging, as dwgsim_hip_fetch: the copy of chunk k+1 overlaps the host copy of chunk k
    const size_t CH = (size_t)16 << 20;
    HIPC(c, c->h_stage.reserve(2 * CH, 2 * CH));
    uint8_t *stage[2] = {c->h_stage.get<uint8_t>(), c->h_stage.get<uint8_t>() + CH};
    size_t done = 0; int b = 0;
    size_t cur = n < CH ? n : CH;
    HIPC(c, hipMemcpyAsync(stage[0], src, cur, hipMemcpyDeviceToHost, c->hap_stream.get()));
    while (done < n) {
        HIPC(c, hipStreamSynchronize(c->hap_stream.get()));
        const size_t next_off = done + cur, next = next_off < n ? ((n - next_off) < CH ? (n - next_off) : CH) : 0;
        if (next) HIPC(c, hipMemcpyAsync(stage[b ^ 1], src + next_off, next, hipMemcpyDeviceToHost, c->hap_stream.get()));
        memcpy((uint8_t *)host_dst + done, stage[b], cur);
        done += cur; cur = next; b ^= 1;
    }
    return DWGSIM_HIP_OK;
}

// ---- the map between a finished haplotype and the reference (dw_walk.hip k_hapchain_count / k_hapchain_write) ----
// On the walk stream, behind the group's walk: block ends per block of cells, their scan, the entries -- into a buffer sized from the scan's total, which the
// device made -- and their copy to the host, which pairs them: the entries of a contig are its blocks' first and last cells in turn.
int dwgsim_hip_haplotype_chain(dwgsim_hip_ctx_t *c, int contig, int hap, uint64_t *blocks)
{
    Group *gp = get_group(c, contig);
    if (!gp) return DWGSIM_HIP_ERR_ARG;
    Group &g = *gp;
    if (hap < 0 || hap > 1) { c->err = "haplotype_chain: hap must be 0 or 1"; return DWGSIM_HIP_ERR_ARG; }
    if (!g.mutated || g.walk_pending) { c->err = "mutate_contig must run first"; return DWGSIM_HIP_ERR_STATE; }
    Group::HapChain &T = g.hap_chain[hap];
    if (!T.valid) {
        HIPC(c, hipSetDevice(c->device));
        GroupMem &M = g.mem;
        hipStream_t st = c->walk_stream.get();
        const size_t n = g.m.size();
        const uint32_t nblk = (uint32_t)((g.total + SCAN_POS_PER_BLOCK - 1) / SCAN_POS_PER_BLOCK);
        if (ensure(c, c->scratch_cnt, ((size_t)nblk + 1) * sizeof(uint32_t))) return DWGSIM_HIP_ERR_DEVICE;
        uint32_t *d_cnt = c->scratch_cnt.get<uint32_t>();
        HapDev hd[2]; fill_haps(g, hd);
        const SegTab seg = seg_tab(g);
        std::vector<uint32_t> pre((size_t)nblk + 1, 0);      // entries in front of every block, and (the last one) of the group: at most two per cell, below 2^32
        std::vector<ChainEnt> ent;
        for (DevEvent &e : c->chain_ev) HIPC(c, e.create());
        c->dbg.chain_count_us = c->dbg.chain_write_us = 0;
        if (nblk) {
            HIPC(c, hipMemsetAsync(d_cnt + nblk, 0, sizeof(uint32_t), st));
            HIPC(c, hipEventRecord(c->chain_ev[0].get(), st));
            launch_hapchain_count(st, hd[hap], seg, g.total, d_cnt);
            launch_scan_excl(st, d_cnt, nblk + 1, nullptr);
            HIPC(c, hipEventRecord(c->chain_ev[1].get(), st));
            HIPC(c, hipMemcpyAsync(pre.data(), d_cnt, ((size_t)nblk + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPC(c, hipStreamSynchronize(st));
            const uint32_t total = pre[nblk];
            ent.resize(total);
            if (total) {
                if (ensure(c, M.d_hap_chain[hap], sizeof(ChainEnt) * (size_t)total)) return DWGSIM_HIP_ERR_DEVICE;
                HIPC(c, hipEventRecord(c->chain_ev[2].get(), st));
                launch_hapchain_write(st, hd[hap], seg, g.total, d_cnt, M.d_hap_chain[hap].get<ChainEnt>(), total);
                HIPC(c, hipEventRecord(c->chain_ev[3].get(), st));
                HIPC(c, hipGetLastError());
                HIPC(c, hipMemcpyAsync(ent.data(), M.d_hap_chain[hap].get(), sizeof(ChainEnt) * (size_t)total, hipMemcpyDeviceToHost, st));
                HIPC(c, hipStreamSynchronize(st));
            }
            float ms = 0;      // (analysis: dwgsim_hip_debug_get "chain_count_us" / "chain_write_us", of the chain built last)
            c->dbg.chain_count_us = hipEventElapsedTime(&ms, c->chain_ev[0].get(), c->chain_ev[1].get()) == hipSuccess ? 1e3 * ms : 0;
            c->dbg.chain_write_us = total && hipEventElapsedTime(&ms, c->chain_ev[2].get(), c->chain_ev[3].get()) == hipSuccess ? 1e3 * ms : 0;
            (void)hipGetLastError();
        }
        T.first.assign(n + 1, 0); T.ref_start.assign(n, 0); T.blocks.clear(); T.blocks.reserve(ent.size() / 2);
        for (size_t k = 0; k < n; ++k) {
            const Member &m = g.m[k];
            const size_t b0 = (size_t)(m.start / SCAN_POS_PER_BLOCK), b1 = m.l > 0 ? (size_t)((m.start + m.l + SCAN_POS_PER_BLOCK - 1) / SCAN_POS_PER_BLOCK) : b0;
            const size_t e0 = pre[b0], e1 = pre[b1];
            T.first[k] = T.blocks.size();
            bool fine = (e1 - e0) % 2 == 0;
            for (size_t q = e0; fine && q < e1; q += 2) {
                const ChainEnt &s = ent[q], &e = ent[q + 1];
                fine = s.info == 0 && (e.info & CHAIN_END) && s.pos <= e.pos && (int64_t)e.pos < m.l && (q == e0 || ent[q - 1].pos < s.pos);
                if (!fine) break;
                if (q == e0) T.ref_start[k] = s.pos; else T.blocks.back().d_ref = (int64_t)s.pos - (int64_t)ent[q - 1].pos - 1;
                T.blocks.push_back(dwgsim_hip_chain_block_t{(int64_t)e.pos - (int64_t)s.pos + 1, m.l - (int64_t)e.pos - 1, (int64_t)(e.info & ~CHAIN_END)});
            }
            if (!fine) { c->err = "haplotype_chain: the block ends of contig '" + m.name + "' do not pair up"; return DWGSIM_HIP_ERR_DEVICE; }
        }
        T.first[n] = T.blocks.size();
        T.valid = true;
    }
    c->dbg.chain_blocks = (int64_t)T.blocks.size();
    if (blocks) *blocks = T.blocks.size();
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_chain_blocks(dwgsim_hip_ctx_t *c, int contig, int hap, uint64_t *n, int64_t *ref_start, dwgsim_hip_chain_block_t *blocks, uint64_t cap)
{
    int km = 0;
    Group *gp = get_group(c, contig, &km);
    if (!gp) return DWGSIM_HIP_ERR_ARG;
    if (hap < 0 || hap > 1 || (!blocks && cap)) { c->err = "chain_blocks: hap must be 0 or 1, and a capacity needs an array"; return DWGSIM_HIP_ERR_ARG; }
    const Group::HapChain &T = gp->hap_chain[hap];
    if (!T.valid) { c->err = "chain_blocks: dwgsim_hip_haplotype_chain must run first"; return DWGSIM_HIP_ERR_STATE; }
    const uint64_t f = T.first[(size_t)km], cnt = T.first[(size_t)km + 1] - f;
    if (n) *n = cnt;
    if (ref_start) *ref_start = T.ref_start[(size_t)km];
    if (cnt && cap) memcpy(blocks, T.blocks.data() + f, sizeof(dwgsim_hip_chain_block_t) * (size_t)(cnt < cap ? cnt : cap));
    return DWGSIM_HIP_OK;
}

// The one formatter of a chain: the command line, the job and Python write these bytes
int64_t dwgsim_hip_chain_format(const char *name, int64_t l, int64_t ref_start, const dwgsim_hip_chain_block_t *blocks, uint64_t n, int direction, uint64_t id, char *buf, size_t cap)
{
    if (!name || !blocks || n == 0 || (direction != DWGSIM_HIP_CHAIN_TO_REF && direction != DWGSIM_HIP_CHAIN_FROM_REF) || ref_start < 0) return DWGSIM_HIP_ERR_ARG;
    int64_t score = 0, ref = ref_start, hap = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const dwgsim_hip_chain_block_t &b = blocks[k];
        if (b.size <= 0 || b.d_ref < 0 || b.d_hap < 0 || (k + 1 < n && b.d_ref == 0 && b.d_hap == 0)) return DWGSIM_HIP_ERR_ARG;
        score += b.size; ref += b.size + b.d_ref; hap += b.size + b.d_hap;
    }
    if (ref != l) return DWGSIM_HIP_ERR_ARG;
    const dwgsim_hip_chain_block_t &z = blocks[n - 1];
    const bool from_ref = direction == DWGSIM_HIP_CHAIN_FROM_REF;
    std::string t = "chain " + std::to_string(score);
    for (int side = 0; side < 2; ++side) {
        const bool is_ref = (side == 0) == from_ref;
        t += ' '; t += name; t += ' ';
        if (is_ref) t += std::to_string(l) + " + " + std::to_string(ref_start) + " " + std::to_string(l - z.d_ref);
        else t += std::to_string(hap) + " + 0 " + std::to_string(hap - z.d_hap);
    }
    t += ' '; t += std::to_string(id); t += '\n';
    char num[80];
    for (uint64_t k = 0; k + 1 < n; ++k) {
        const dwgsim_hip_chain_block_t &b = blocks[k];
        const int w = snprintf(num, sizeof num, "%lld\t%lld\t%lld\n", (long long)b.size, (long long)(from_ref ? b.d_ref : b.d_hap), (long long)(from_ref ? b.d_hap : b.d_ref));
        t.append(num, (size_t)w);
    }
    t += std::to_string(z.size); t += "\n\n";
    if (buf && cap >= t.size()) memcpy(buf, t.data(), t.size());
    return (int64_t)t.size();
}

// ---- read simulation ----
namespace {
// One launch over a list of ranges (sim_resolve): form, group, range table with its pairs, blocks and longest "[prefix_]name", arguments
struct Launch { SimForm f; SimArgs a; Group *g = nullptr; std::vector<SimSeg> segs; uint64_t n_pairs = 0; uint32_t nblk = 0; int fixed_max = 0; };
// The sizes of one k_simulate launch besides its arguments (sim_plan), in bytes -- 0: the launch does not use that buffer -- and what follows from them
struct SimPlan {
    size_t cap[N_STREAMS];                // record capacity of each stream (0: not written); its text buffer holds 64 bytes more
    size_t t_nl[2], t_rec[2], t_ends, t_len, t_blk; int32_t t_qname_max;      // the truth step's working set (0: off)
    int32_t lb_shift; bool too_many;      // SimArgs::lb_shift; the launch's sums would not fit the look-back word of the single Illumina / SOLiD kernel
    size_t block_rand, status, meta, fail_summ, split_state, split_hand, split_agg, split_pre, split_chunk;      // (split_*: what the first half of the two-kernel form hands to the second)
    bool scratch; int32_t flow_slots; size_t flow_scratch, flow_free;      // scratch slots: in use, per XCD, the slots, their free lists
    size_t segs, gz_chunks[N_STREAMS], gz_cap[N_STREAMS], gz_status;      // the range table; GPU gzip: chunks and member capacity of each stream, the look-back words of all
};
struct ChainSet { uint64_t *words; int set_rand, set_carry; uint64_t carry; };      // where a launch's running values come from (launch_init / launch_chain_set)
}

// The ranges of one launch: all of one walked group, in file order.  ppb = pairs per block of the kernel that will run.
static int build_ranges(dwgsim_hip_ctx_t *c, const dwgsim_hip_range_t *r, int n, uint64_t ppb, Launch &L)
{
    if (!r || n < 1) { c->err = "bad range arguments"; return DWGSIM_HIP_ERR_ARG; }
    Group *g = nullptr;
    uint64_t pairs = 0, blocks = 0; int fmax = 0;
    std::vector<SimSeg> &segs = L.segs;
    segs.clear();
    for (int q = 0; q < n; ++q) {
        int k = 0;
        Group *gq = get_group(c, r[q].contig, &k);
        if (!gq) return DWGSIM_HIP_ERR_ARG;
        if (g && gq != g) { c->err = "the ranges of one call must belong to contigs that were added together (dwgsim_hip_add_contigs)"; return DWGSIM_HIP_ERR_ARG; }
        g = gq;
        if (r[q].n_pairs == 0) continue;
        const Member &m = g->m[(size_t)k];
        if (c->has_regions && m.n_reg == 0 && c->prm.rand_read < 1.0) { c->err = "dwgsim-hip: this contig has no target region (-x): the reference's placement loop would not terminate\n"; return DWGSIM_HIP_ERR_ARG; }
        SimSeg s; memset(&s, 0, sizeof s);
        s.first_block = (uint32_t)blocks; s.contig_index = m.contig_index; s.start = m.start; s.l = (int32_t)m.l;
        s.first_ii = r[q].first_ii; s.n_pairs = r[q].n_pairs; s.pair_off = pairs; s.l_place = m.l_place;
        s.reg_off = m.reg_off; s.n_reg = m.n_reg; s.name_off = m.name_off; s.name_fixed_len = m.name_fixed_len;
        s.contig_start = r[q].first_ii == 0 ? 1u : 0u;
        segs.push_back(s);
        pairs += r[q].n_pairs; blocks += (r[q].n_pairs + ppb - 1) / ppb;
        if (m.name_fixed_len > fmax) fmax = m.name_fixed_len;
        if (blocks > 0x7fffffffull) { c->err = "too many pairs in one call"; return DWGSIM_HIP_ERR_ARG; }
    }
    if (!g->mutated || g->walk_pending) { c->err = "mutate_contig must run first"; return DWGSIM_HIP_ERR_STATE; }
    L.g = g; L.n_pairs = pairs; L.nblk = (uint32_t)blocks; L.fixed_max = fmax;
    return DWGSIM_HIP_OK;
}

// The k_simulate form of a launch (dw_kernels.hpp SimForm): the one place that decides it, from the options, the base-quality tables, the Ion Torrent
// capacity multiplier and the debug overrides ("writer", "sim_threads", "split", "ion_lds", "flow_cap").  Sets c->err when the reads cannot be run.
static int sim_form(dwgsim_hip_ctx_t *c, SimForm &f)
{
    const dwgsim_hip_params_t &p = c->prm;
    const size_t qb = (size_t)c->tab.qb_words;
    const int lmax = p.length[0] > p.length[1] ? p.length[0] : p.length[1];
    f = SimForm();
    f.lpp = p.length[1] > 0 ? 2 : 1;
    f.out = (p.reads_output_type != 2 ? 1 : 0) | (p.reads_output_type != 1 ? 2 : 0);
    f.dt = p.data_type;
    // lanes per k_simulate block: the staged read (lds_words per lane) must fit LDS; long Illumina / SOLiD reads get one-wave blocks
    f.nthr = SIM_THREADS;
    f.cap = lmax; f.lds_words = (lmax + 7) / 8;
    // the FIFO writer unless its LDS costs a resident block per CU (Illumina reads between ~150 and ~240 bases): then 16-byte pieces from registers
    bool fifo = true;
    if (p.data_type == 0) {
        // waves per SIMD the registers allow (k_simulate launch bounds): five, except with both output families (-o 0) through two register writers;
        // through the FIFO both families leave from one image (dw_read.hpp FifoWriter DUAL) and the kernel needs no more registers than for one
        const int cap_fifo = 5, cap_reg = (p.reads_output_type == 0) ? 4 : 5;
        const int b_fifo = sim_blocks_per_cu(sim_lds_bytes((size_t)f.lds_words, SIM_THREADS, qb, true), cap_fifo), b_reg = sim_blocks_per_cu(sim_lds_bytes((size_t)f.lds_words, SIM_THREADS, qb, false), cap_reg);
        // (-o 0: one assembly for both families outweighs a resident block: 2 x 250 bp 7.72 ms with three blocks per CU against 8.13 ms with four, profiles/r05_o0.txt)
        if (b_fifo < b_reg && !(p.reads_output_type == 0 && b_fifo >= 3)) fifo = false;
        if (c->dbg.writer >= 0) fifo = c->dbg.writer != 0;
    }
    const size_t need = sim_lds_bytes((size_t)f.lds_words, SIM_THREADS, qb, fifo);     // staged bases + the two base-quality tables + the text FIFOs
    // (from where LDS staging leaves room for ONE 256-lane block per CU -- reads of ~650 bases on -- the one-wave blocks are the faster form: 800 / 1 000 /
    // 2 000 bases 13.1 / 13.0 / 22.7 ms in LDS against 7.8 / 8.0 / 8.6 ms staged in scratch slots, 600 bases 7.4 against 7.9: profiles/r04_long_reads.txt)
    if (p.data_type != 2 && (need > SIM_LDS_BUDGET || ((sim_blocks_per_cu(need, 8) < 2 || c->dbg.force_threads == SIM_THREADS_LONG) && c->dbg.force_threads != SIM_THREADS))) {
        // reads too long to stage in LDS: one-wave blocks whose reads are staged in scratch slots (global memory, dw_simulate.hip GS); what is left in LDS
        // is the two base-quality tables (2 bytes per base) and the FIFOs, which bounds a read at ~70 000 bases (the reference has no bound, dwgsim.c:75-153)
        f.nthr = SIM_THREADS_LONG; fifo = true;
        if (sim_lds_bytes(0, SIM_THREADS_LONG, qb, true) > SIM_LDS_BUDGET) {
            char b[160]; snprintf(b, sizeof b, "dwgsim-hip: reads longer than %d bases are not supported for -c 0 / -c 1\n", (int)((SIM_LDS_BUDGET - SIM_THREADS_LONG * SIM_FIFO_BYTES) / 2 - 16));
            c->err = b; return DWGSIM_HIP_ERR_UNSUP;
        }
    }
    if (p.data_type == 2) {        // room for flow-space insertions: ~2.4 empty flows per base, each inserting with probability e, plus cascades
        f.cap = std::max(flow_base_capacity(c), lmax) * c->flow_cap_mult;      // (the read as extracted must fit: a forced capacity is a test's starting point, never below the read length)
        // the flow model's one in-place buffer per lane, 2 bits per base (dw_read.hpp flow_errors), and the run stack of its pass 2.  In LDS while at
        // least two 256-lane blocks -- or else four one-wave blocks -- fit a CU; beyond that (very long reads, error rates at which reads grow
        // severalfold) in scratch slots of global memory ("ion_lds": 0 slots, 1 / 2 LDS with 256 / 64 lanes, -1 choose)
        f.lds_words = (f.cap + 15) / 16; f.cap = 16 * f.lds_words;
        f.stack_words = std::min(FLOW_STACK_WORDS * c->flow_cap_mult, FLOW_STACK_WORDS_MAX);
        const size_t per_lane = (size_t)(f.lds_words + f.stack_words);
        const size_t need256 = sim_lds_bytes(per_lane, SIM_THREADS, qb, true), need64 = sim_lds_bytes(per_lane, ION_THREADS_SMALL, qb, true);
        int mode = c->dbg.ion_lds;
        if (mode < 0) mode = (need256 <= SIM_LDS_BUDGET && sim_blocks_per_cu(need256, 8) >= 2) ? 1 : (need64 <= SIM_LDS_BUDGET && sim_blocks_per_cu(need64, 32) >= 4) ? 2 : 0;
        if ((mode == 1 && need256 > SIM_LDS_BUDGET) || (mode == 2 && need64 > SIM_LDS_BUDGET)) mode = 0;
        f.dt = mode != 0 ? 3 : 2; f.nthr = mode == 2 ? ION_THREADS_SMALL : SIM_THREADS;
    }
    // Short Illumina reads run as two kernels with the offsets computed in between (dw_simulate.hip SPLIT): no look-backs, and the second half --
    // no staged bases in LDS -- writes the text in 64-byte bursts: what does not scale with the read length (placement, the look-backs, the name) is most of the
    // work of short reads.  Against the single kernel with ONE look-back (dw_simulate.hip ONE_LB; profiles/r06_bench_lines_final.txt 14): 2 x 36 bp +5.5 % as
    // two kernels, 2 x 50 +0.8 %, 2 x 75 -3 %, 2 x 100 -10 %, 100 bp single-end -9 %, 2 x 150 -12 %.  "split" = 0 / 1 forces either.
    // (The cut at 100 bases of rounds 4-5 and their rule for small launches: DESIGN.md §4, k_simulate.)
    const bool split_wins = lmax <= 50;
    f.split = (p.data_type == 0 && f.nthr == SIM_THREADS && (c->dbg.split < 0 ? split_wins : c->dbg.split != 0)) ? 1 : 0;
    // Ion Torrent with its buffers in LDS: as two kernels as well (the flow model | qualities + text).  The first half holds no text FIFOs, so a fourth
    // block fits a CU, and no block waits for the record sizes of the blocks in front of it ("split" = 0 forces the single kernel)
    if (f.dt == 3 && f.nthr == SIM_THREADS && f.cap < 32768 && c->dbg.split != 0) f.split = 1;
    if (f.split && c->dbg.writer < 0) fifo = true;      // (its LDS holds no bases: the FIFO writer always fits)
    // dynamic LDS: the staged bases (Ion Torrent: the read buffers when LDS holds them + the pass-2 run stack; the scratch slots hold the rest, and the
    // reads of the one-wave blocks) + the base-quality tables + the text FIFOs.  Two kernels: the first half stages the bases only, the second half
    // (no staged bases) the tables and its FIFOs of 64-byte bursts
    const size_t stage = f.dt == 3 ? (size_t)(f.lds_words + f.stack_words) : f.dt == 2 ? (size_t)f.stack_words : f.nthr != SIM_THREADS ? 0 : (size_t)f.lds_words;
    if (f.split) { f.wr = fifo ? 2 : 0; f.lds = sim_lds_bytes(stage, (size_t)f.nthr, 0, false); f.lds_b = sim_lds_bytes(0, (size_t)f.nthr, qb, fifo, SIM_FIFO_BYTES_WIDE); }
    else { f.wr = fifo ? 1 : 0; f.lds = sim_lds_bytes(stage, (size_t)f.nthr, qb, fifo); }
    return 0;
}

// The arguments of a launch of form f over group g that do not depend on its ranges (sim_plan and the enqueue step add those)
static void fill_sim_args(const dwgsim_hip_ctx_t *c, const Group &g, const SimForm &f, SimArgs &a)
{
    const dwgsim_hip_params_t &p = c->prm;
    memset(&a, 0, sizeof a);
    a.p.std_dev = p.std_dev; a.p.mut_freq = p.mut_freq; a.p.rand_read = p.rand_read; a.p.quality_std = p.quality_std;
    a.p.dist = p.dist; a.p.is_inner = p.is_inner; a.p.len[0] = p.length[0]; a.p.len[1] = p.length[1]; a.p.max_n = p.max_n;
    a.p.strandedness = p.strandedness; a.p.read_one_strand = p.read_one_strand; a.p.amplicons = p.amplicons;
    a.p.fixed_quality = p.fixed_quality; a.p.data_type = p.data_type;
    a.p.has_bfast = p.reads_output_type != 1; a.p.has_bwa = p.reads_output_type != 2;
    a.p.seed = (uint32_t)p.seed;
    lazy_quality_params(p.quality_std, &a.p.q_k, &a.p.q_eps, &a.p.q_lmin, &a.p.q_near1);
    fill_haps(g, a.hap);
    a.chain = c->d_chain.get<uint64_t>();
    a.have_regions = c->has_regions ? 1 : 0; a.reg = g.mem.d_reg.get<int32_t>();
    for (int j = 0; j < 2; ++j) { a.e_thr[j] = c->tab.d_thr[j].get<uint64_t>(); a.e_thr32[j] = c->tab.d_thr32[j].get<uint32_t>(); a.qbase[j] = c->tab.d_qbase[j].get<uint32_t>() ? c->tab.d_qbase[j].get<uint32_t>() : c->tab.d_qbase[0].get<uint32_t>(); }
    a.qb_words = c->tab.qb_words;
    a.e_full = c->tab.e_full;
    a.names = g.mem.d_names.get();
    a.summ[0] = g.mem.d_summ[0].get<uint16_t>(); a.summ[1] = g.mem.d_summ[1].get<uint16_t>(); a.summ2[0] = g.mem.d_summ2[0].get<uint16_t>(); a.summ2[1] = g.mem.d_summ2[1].get<uint16_t>();
    // k_place decides most pairs without their insert size: |normal| <= sqrt(-2 ln 2^-104) < 12.01 for the polar method on 53-bit uniforms (dw_simulate.hip pair_surely_accepted)
    a.place_fast = (!c->has_regions && !p.amplicons && p.std_dev * 12.1 + 2.0 < 1e9) ? 1 : 0;
    a.place_k = a.place_fast ? (int32_t)ceil(p.std_dev * 12.1) + 2 : 0;
    a.rand_fixed = c->tab.d_rand_fixed.get(); a.rand_fixed_len = c->tab.rand_fixed_len;
    a.sim_threads = f.nthr; a.fifo = f.wr != 0; a.split = f.split; a.ion_lds = f.dt == 3;
    a.cap = f.cap; a.lds_words = f.lds_words; a.flow_stack_words = f.stack_words;
    // the quality line in the staging rows: the instances that write the sequence line in lockstep units (dw_simulate.hip SEQ_LOCKSTEP), from 72 bytes per lane on
    a.qrows = (c->dbg.qrows != 0 && f.dt == 0 && f.split == 0 && f.wr == 1 && f.nthr == SIM_THREADS && f.out != 3 && f.lds_words >= 18) ? 1 : 0;
    a.flow = c->tab.d_flow.get(); a.flow_len = (int32_t)c->tab.flow.size();
    for (int j = 0; j < 2; ++j) {      // Illumina / SOLiD: the gap chain of a read end's error sites runs at the largest threshold of its ramp (dw_simulate.hip; thresholds as dwgsim_hip_create made them)
        const int n = c->prm.length[j];
        uint64_t tmax = 0, tmin = ~0ull;
        for (int i = 0; i < n; ++i) {
            const double ei = c->prm.e_start[j] + c->tab.e_by[j] * i;
            const uint64_t t = !(ei > 0) ? 0 : ei >= 1.0 ? 0x100000000ull : (uint64_t)ceil(ei * 4294967296.0);
            tmax = std::max(tmax, t); tmin = std::min(tmin, t);
        }
        a.err_thr_max[j] = n > 0 ? tmax : 0; a.err_ramp[j] = (n > 0 && tmin != tmax) ? 1 : 0;
        flow_gap_params(a.err_thr_max[j], &a.err_gap_r[j], &a.err_gap_s[j]);
    }
    for (int j = 0; j < 2; ++j) {      // Ion Torrent: the gap draws of the flow model, from the read end's (uniform) threshold as dwgsim_hip_create made it (thr[0])
        const double e0 = c->prm.e_start[j];
        flow_gap_params(!(e0 > 0) ? 0 : e0 >= 1.0 ? 0x100000000ull : (uint64_t)ceil(e0 * 4294967296.0), &a.flow_gap_r[j], &a.flow_gap_s[j]);
    }
}

// The resolve step of a k_simulate launch, in a fixed order: the group of r[0] is known, the form, the range table laid out for the form's pairs per
// block, the arguments for the table's group (r[0]'s: build_ranges refuses ranges of two groups).
static int sim_resolve(dwgsim_hip_ctx_t *c, const dwgsim_hip_range_t *r, int n, Launch &L)
{
    if (!r || n < 1) { c->err = "bad range arguments"; return DWGSIM_HIP_ERR_ARG; }
    if (!get_group(c, r[0].contig)) return DWGSIM_HIP_ERR_ARG;
    if (const int rc = sim_form(c, L.f)) return rc;
    if (const int rc = build_ranges(c, r, n, (uint64_t)(L.f.nthr / L.f.lpp), L)) return rc;
    fill_sim_args(c, *L.g, L.f, L.a);
    return DWGSIM_HIP_OK;
}

// the reference's own last words (dwgsim.c:833-843): one pair used up its 10 001 attempts, or the counter of failed attempts over the pairs of a contig passed the limit (dwgsim.c:635)
static int fail_attempts(dwgsim_hip_ctx_t *c) { char b[128]; snprintf(b, sizeof b, "\r[dwgsim_core] failed to generate a read after %d trials\n", MAX_ATTEMPTS + 1); c->err = b; return DWGSIM_HIP_ERR_FAILED; }
int dwgsim_hip_count_random_ranges(dwgsim_hip_ctx_t *c, const dwgsim_hip_range_t *r, int n, uint64_t *n_random, uint64_t *per_range)
{
    if (!c) return DWGSIM_HIP_ERR_ARG;
    if (n_random) *n_random = 0;
    if (per_range) for (int q = 0; q < n; ++q) per_range[q] = 0;
    // the resolve step of sim_resolve in the count's order: k_place's range table does not depend on the form, so bad ranges are reported first, a
    // count without pairs is no error, and the form is taken behind the group's walk
    Launch L;
    if (const int rc = build_ranges(c, r, n, PLACE_PAIRS, L)) return rc;
    const uint64_t n_pairs = L.n_pairs; const uint32_t n_blocks = L.nblk;
    if (n_pairs == 0) return DWGSIM_HIP_OK;
    Group &g = *L.g;
    HIPC(c, hipSetDevice(c->device));
    hipStream_t st = c->count_stream.get();     // (the count of one group can run while batches of another -- or of this one -- are being simulated)
    // (the haplotype summaries k_place reads -- per 64 and per 1024 cells -- were written with the read views at the end of the walk: the count follows
    // its group's walk by that walk's event, whatever else has been put on the walk stream since)
    if (g.walk_pending) { if (const int rc = dwgsim_hip_mutate_wait(c, g.first_handle)) return rc; }      // (a walk that exceeded a capacity is run again inside the wait: only then are the summaries final)
    if (g.mem.ev_walk.get() && g.mutated) HIPC(c, hipStreamWaitEvent(st, g.mem.ev_walk.get(), 0));
    if (const int rc = sim_form(c, L.f)) return rc;
    SimArgs &a = L.a; fill_sim_args(c, g, L.f, a);
    const size_t ns = L.segs.size();
    if (ensure(c, c->place_rand, sizeof(uint32_t) * ((size_t)n_blocks + 1)) || ensure(c, c->place_segs, sizeof(SimSeg) * ns) ||
        ensure(c, c->place_aux, PLACE_LISTS * 16 * sizeof(uint32_t) + sizeof(uint64_t) * ns)) return DWGSIM_HIP_ERR_DEVICE;
    if (sizeof(SimSeg) * ns > c->h_place_segs.cap() || sizeof(uint64_t) * ns > c->h_range_rand.cap()) HIPC(c, hipStreamSynchronize(st));      // (before the page-locked pair is replaced)
    HIPC(c, c->h_place_segs.reserve(sizeof(SimSeg) * ns, sizeof(SimSeg) * (ns + 64))); HIPC(c, c->h_range_rand.reserve(sizeof(uint64_t) * ns, sizeof(uint64_t) * (ns + 64)));
    const uint64_t *h_range_rand = c->h_range_rand.get<uint64_t>();
    memcpy(c->h_place_segs.get(), L.segs.data(), sizeof(SimSeg) * ns);
    HIPC(c, hipMemcpyAsync(c->place_segs.get(), c->h_place_segs.get(), sizeof(SimSeg) * ns, hipMemcpyHostToDevice, st));
    a.segs = c->place_segs.get<SimSeg>(); a.n_seg = (int32_t)ns; a.n_blocks = n_blocks; a.n_pairs = n_pairs;
    a.block_rand = c->place_rand.get<uint32_t>(); a.counters = c->pcounters.dev();
    // the lists of pairs k_place leaves open: room for an eighth of the pairs (the usual share is a per cent); if that does not do -- contigs
    // made of N runs, a read length close to the contig's -- the count is run once more with room for every pair
    const uint64_t waves = (uint64_t)n_blocks * (PLACE_PAIRS / 64);
    const uint32_t cap_full = (uint32_t)((waves + PLACE_LISTS - 1) / PLACE_LISTS) * 64u;
    uint32_t cap = (uint32_t)std::min<uint64_t>(cap_full, 1024 + n_pairs / PLACE_LISTS / 8);
    if (c->dbg.place_cap >= 0 && (uint64_t)c->dbg.place_cap < cap) cap = (uint32_t)c->dbg.place_cap;      // dwgsim_hip_debug_option("place_cap"): start too small, exercise the second run
    for (int attempt = 0;; ++attempt) {
        if (ensure(c, c->place_list, sizeof(uint32_t) * (size_t)cap * PLACE_LISTS)) return DWGSIM_HIP_ERR_DEVICE;
        a.place_list = c->place_list.get<uint32_t>(); a.place_list_cap = cap;
        a.place_list_n = c->place_aux.get<uint32_t>(); a.range_rand = reinterpret_cast<uint64_t *>(c->place_aux.get<uint8_t>() + PLACE_LISTS * 16 * sizeof(uint32_t));
        HIPC(c, hipMemsetAsync(c->pcounters.dev(), 0, N_COUNTERS * sizeof(uint64_t), st));
        HIPC(c, hipMemsetAsync(c->place_aux.get(), 0, PLACE_LISTS * 16 * sizeof(uint32_t) + sizeof(uint64_t) * ns, st));
        HIPC(c, hipEventRecord(c->ev_cnt0.get(), st));
        launch_place(st, a);
        HIPC(c, hipEventRecord(c->ev_cnt1.get(), st));
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(c->pcounters.host(), c->pcounters.dev(), N_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIPC(c, hipMemcpyAsync(c->h_range_rand.get(), a.range_rand, sizeof(uint64_t) * ns, hipMemcpyDeviceToHost, st));
        HIPC(c, hipStreamSynchronize(st));
        { float ms = 0; if (hipEventElapsedTime(&ms, c->ev_cnt0.get(), c->ev_cnt1.get()) == hipSuccess) c->dbg.count_us += 1e3 * ms; else (void)hipGetLastError(); }
        if (!(c->pcounters.host()[STATUS_COUNTER] & PLACE_ROOM_BIT) || attempt > 0) break;
        cap = cap_full;
    }
    if (c->pcounters.host()[STATUS_COUNTER] & PLACE_ROOM_BIT) { c->err = "count_random: the list of undecided pairs overflowed twice"; return DWGSIM_HIP_ERR_FAILED; }
    if (c->pcounters.host()[STATUS_COUNTER]) return fail_attempts(c);
    c->dbg.place_open = c->pcounters.host()[PLACE_OPEN_COUNTER];
    uint64_t total = 0;
    for (int q = 0, si = 0; q < n; ++q) if (r[q].n_pairs) { total += h_range_rand[si]; if (per_range) per_range[q] = h_range_rand[si]; ++si; }
    if (n_random) *n_random = total;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_count_random(dwgsim_hip_ctx_t *c, int contig, uint64_t first_ii, uint64_t n_pairs, uint64_t *n_random)
{
    dwgsim_hip_range_t r; memset(&r, 0, sizeof r); r.contig = contig; r.first_ii = first_ii; r.n_pairs = n_pairs;
    return dwgsim_hip_count_random_ranges(c, &r, 1, n_random, nullptr);
}

int dwgsim_hip_set_fail_carry(dwgsim_hip_ctx_t *c, uint64_t carry)
{
    if (!c) return DWGSIM_HIP_ERR_ARG;
    c->carry_override = carry; c->has_carry_override = true;
    return DWGSIM_HIP_OK;
}

// How a batch is run: where its random-read index starts (DWGSIM_HIP_RAND_CHAIN: where the last batch ended).  again: the batch of this slot once more (sim_rerun), with
// truth_bytes of room for its truth SAM (0: the planned bound).  Nothing of the chain moves then: the random reads and the failed attempts of a batch depend on no buffer's size,
// so the first run's epilogue stands; the kernels start from the chain word the first run started from (rand_base = its CHAIN_BASE_COUNTER).
struct SimRun { uint64_t rand_base; bool again; uint64_t truth_bytes; };

// The plan step: every size the launch needs, from its form, arguments and ranges.  No side effects.
static SimPlan sim_plan(const dwgsim_hip_ctx_t *c, const Launch &L, const SimRun &run)
{
    const dwgsim_hip_params_t &p = c->prm; const SimForm &f = L.f;
    const uint64_t n_pairs = L.n_pairs; const size_t nblk = L.nblk;
    SimPlan P{};
    // upper bound of one FASTQ record (name tail: 2 positions <= 10 digits, 6 counters, 16 hex digits)
    const int fixed_max = std::max(L.fixed_max, c->tab.rand_fixed_len);
    for (int j = 0; j < 2; ++j) if (p.length[j] > 0) P.cap[j] = (size_t)n_pairs * (size_t)(1 + fixed_max + 120 + 3 + 2 * (p.data_type == 2 ? f.cap : p.length[j]) + 4);
    // the one look-back word of the single Illumina kernel: 62 bits for the random reads and the bytes of stream 1 in front of a block
    int bw_bytes = 0, bw_pairs = 0;
    while (bw_bytes < 63 && (((uint64_t)P.cap[0] | 1ull) >> bw_bytes)) ++bw_bytes;
    while (bw_pairs < 63 && (n_pairs >> bw_pairs)) ++bw_pairs;
    P.lb_shift = bw_bytes; P.too_many = p.data_type != 2 && bw_bytes + bw_pairs > 62;      // (Illumina and SOLiD; at 2 x 150 bp: more than 2^26 pairs)
    P.cap[2] = P.cap[0] + P.cap[1];
    if (!L.a.p.has_bwa) P.cap[0] = P.cap[1] = 0;
    if (!L.a.p.has_bfast) P.cap[2] = 0;
    if (c->depth_on && !c->truth_on) { size_t ends = 0; for (int j = 0; j < 2; ++j) if (p.length[j] > 0) ends += n_pairs; P.t_ends = sizeof(TruthEnd) * ends; }      // the true read depth alone: the read ends, nothing else of the truth step
    if (c->truth_on) {
        // The truth SAM (dw_truth.hpp), sized here so that no length crosses to the host.  A line of a read end of s bases is at most
        //   QNAME (the FASTQ name without '@': below fixed_max + 120, the bound the FASTQ buffers are sized with) + FLAG (3) + RNAME (fixed_max) + POS (10) + MAPQ (2)
        //   + CIGAR + RNEXT (1) + PNEXT (10) + TLEN (11) + SEQ (s) + QUAL (s) + "HP:i:1" (6) + 11 tabs + the newline.
        // CIGAR: the runs that hold read bases (M, I) have counts of at least one each that add up to s -- at most s runs, and a count has no more digits than
        // its value: 2 s characters at most.  A D run stands between two read bases (never first or last) and neighbouring ones merge: at most s - 1 of them, each
        // a count below 2^31 (10 digits) and its letter.  Together at most 2 s + 11 (s - 1) < 13 s.  (1M1D1M1D... takes 4 s - 2.)
        P.t_qname_max = fixed_max + 120;
        size_t ends = 0, bytes = 0;
        for (int j = 0; j < 2; ++j) if (p.length[j] > 0) { ends += n_pairs; bytes += (size_t)n_pairs * (size_t)(P.t_qname_max + fixed_max + 3 + 10 + 2 + 1 + 10 + 11 + 6 + 11 + 1 + 15 * (size_t)p.length[j]); }
        // NM and MD (dwgsim_hip_set_truth_md): the part that IS bounded -- two tabs, "NM:i:" and "MD:Z:" (12), NM's digits (10), and for the M cells, at most s of
        // them, a count and a letter each and the last count: 2 s + 1.  MD also spells out every deleted base, and a -m file may delete kilobases between two
        // read bases: no bound in s exists.  The lines pack contiguously, so those bases normally come out of the slack of the 15 s above; where they do not, the
        // write pass says so and dwgsim_hip_wait runs the batch again with the exact size (SimRun::truth_bytes).
        if (c->truth_md) for (int j = 0; j < 2; ++j) if (p.length[j] > 0) bytes += (size_t)n_pairs * (size_t)(12 + 10 + 2 * (size_t)p.length[j] + 1);
        if (run.truth_bytes) bytes = (size_t)run.truth_bytes;
        else if (c->dbg.truth_cap >= 0 && c->truth_md) bytes = (size_t)std::max<int64_t>(c->dbg.truth_cap, 64);      // dwgsim_hip_debug_option("truth_cap"): start too small, exercise the second run
        P.cap[3] = bytes;
        const bool bfast_src = !L.a.p.has_bwa;
        for (int q = 0; q < (bfast_src ? 1 : f.lpp); ++q) {
            const size_t src_cap = P.cap[bfast_src ? 2 : q];
            P.t_nl[q] = sizeof(uint32_t) * ((src_cap + 4095) / 4096 + 1); P.t_rec[q] = sizeof(uint32_t) * ((bfast_src ? ends : (size_t)n_pairs) + 2);
        }
        P.t_ends = sizeof(TruthEnd) * ends; P.t_len = sizeof(uint32_t) * (ends + 1); P.t_blk = sizeof(uint32_t) * (nblk + 1);
        for (int t = 0; t < N_STREAMS; ++t) if ((uint64_t)P.cap[t] >> 32) P.too_many = true;      // (record starts and line starts are 32-bit words)
    }
    P.block_rand = sizeof(uint32_t) * nblk;
    if (!f.split) P.status = 4 * sizeof(uint64_t) * nblk;      // the four look-back arrays, contiguous: one memset per batch
    else { P.split_state = sizeof(uint32_t) * (size_t)f.lds_words * SIM_THREADS * nblk; P.split_hand = 16 * (size_t)SIM_THREADS * nblk; P.split_agg = 16 * nblk; P.split_pre = 32 * nblk; P.split_chunk = 32 * (nblk / 1024 + 1); }
    P.meta = sizeof(uint32_t) * ((size_t)n_pairs + 8);      // (+ padding for 16-byte reads)
    P.fail_summ = ((size_t)((n_pairs + 256ull * 64 - 1) / (256ull * 64)) * 4 + 2) * sizeof(uint64_t);
    P.scratch = f.dt == 2 || (f.dt < 2 && f.nthr == SIM_THREADS_LONG);
    if (P.scratch) {
        // read buffers (Ion Torrent) / staged reads (one-wave blocks): one slot per block an XCD can hold at a time -- what the LDS admits per CU, at most the eight waves of a SIMD (registers can only
        // lower it; too few slots would make blocks wait, never fail) --, handed from block to block inside the XCD (dw_simulate.hip scratch_slot_take)
        const int cu_per_xcd = (c->n_cu >= 64 && c->n_cu % 8 == 0) ? c->n_cu / 8 : c->n_cu;
        const bool ion = p.data_type == 2;
        const int per_cu = sim_blocks_per_cu(f.lds, ion ? 8 : 32);       // (one-wave blocks: up to eight per SIMD)
        P.flow_slots = c->dbg.flow_slots > 0 ? c->dbg.flow_slots : cu_per_xcd * per_cu;
        if ((uint64_t)P.flow_slots > (uint64_t)nblk) P.flow_slots = (int32_t)nblk;
        if (ion) {      // reads that have grown far beyond their estimate (capacity re-runs): fewer slots, at most 4 GB of them (blocks wait for a slot, they never fail for want of one)
            const size_t slot_bytes = (size_t)flow_words_per_lane(f.lds_words) * (size_t)SIM_THREADS * sizeof(uint32_t);
            const size_t fit = std::max<size_t>(1, ((size_t)4 << 30) / (slot_bytes * 8));
            if ((size_t)P.flow_slots > fit) P.flow_slots = (int32_t)fit;
        }
        const size_t words = (ion ? (size_t)flow_words_per_lane(f.lds_words) * (size_t)SIM_THREADS : (size_t)f.lds_words * (size_t)SIM_THREADS_LONG) * (size_t)P.flow_slots * 8;
        P.flow_scratch = words * sizeof(uint32_t); P.flow_free = sizeof(uint64_t) * (256 + 8 * nblk);
    }
    P.segs = sizeof(SimSeg) * L.segs.size();
    if (c->gzip_on) {
        size_t chunks = 0;
        for (int t = 0; t < N_STREAMS; ++t) { P.gz_chunks[t] = (size_t)gz_chunks(P.cap[t]); chunks += P.gz_chunks[t]; if (P.cap[t]) P.gz_cap[t] = (size_t)gz_capacity(P.cap[t]); }
        P.gz_status = sizeof(uint64_t) * (chunks ? chunks : 1);
    }
    return P;
}

// The reserve step: every buffer grown to its plan (ensure of 0 bytes: nothing), after the wait for a copy of the slot's text still in flight
static int sim_reserve(dwgsim_hip_ctx_t *c, int slot, const SimPlan &P)
{
    Slot &sl = c->slot[slot]; DevMem *out = c->out[slot];
    if (sl.fetch_in_flight) { HIPC(c, hipStreamWaitEvent(c->stream.get(), sl.ev_fetched.get(), 0)); bool grows = false; for (int t = 0; t < N_STREAMS; ++t) if (P.cap[t] + 64 > out[t].cap() && (t < 3 || P.cap[t])) grows = true; if (grows) HIPC(c, hipEventSynchronize(sl.ev_fetched.get())); sl.fetch_in_flight = false; }
    for (int t = 0; t < 3; ++t) if (ensure(c, out[t], P.cap[t] + 64)) return DWGSIM_HIP_ERR_DEVICE;
    if (P.cap[3] && (ensure(c, out[3], P.cap[3] + 64) || ensure(c, c->t_nl[0], P.t_nl[0]) || ensure(c, c->t_nl[1], P.t_nl[1]) || ensure(c, c->t_rec[0], P.t_rec[0]) || ensure(c, c->t_rec[1], P.t_rec[1]) ||
                     ensure(c, c->t_len, P.t_len) || ensure(c, c->t_blk, P.t_blk))) return DWGSIM_HIP_ERR_DEVICE;
    if (ensure(c, c->t_ends, P.t_ends)) return DWGSIM_HIP_ERR_DEVICE;
    if (ensure(c, c->block_rand, P.block_rand) || ensure(c, c->status_all, P.status) ||
        ensure(c, c->split_state, P.split_state) || ensure(c, c->split_hand, P.split_hand) || ensure(c, c->split_agg, P.split_agg) || ensure(c, c->split_pre, P.split_pre) || ensure(c, c->split_chunk, P.split_chunk) ||
        ensure(c, c->meta, P.meta) || ensure(c, c->fail_summ, P.fail_summ) || ensure(c, c->flow_scratch, P.flow_scratch) || ensure(c, c->flow_free, P.flow_free) || ensure(c, sl.segs, P.segs)) return DWGSIM_HIP_ERR_DEVICE;
    HIPC(c, sl.h_segs.reserve(P.segs, P.segs + 64 * sizeof(SimSeg)));      // (+ 64 entries; the slot is not pending: no copy reads the old one)
    for (int t = 0; t < N_STREAMS; ++t) if (P.gz_cap[t] && ensure(c, sl.gz_out[t], P.gz_cap[t] + 64)) return DWGSIM_HIP_ERR_DEVICE;
    return ensure(c, sl.gz_status, P.gz_status);
}

// The chain step: the running values the batch starts from; the context's chain moves on to its end (a re-run moves nothing)
static ChainSet sim_chain(dwgsim_hip_ctx_t *c, Slot &sl, const dwgsim_hip_range_t *r, int n, const SimRun &run)
{
    if (run.again) return ChainSet{sl.d_rerun_chain.get<uint64_t>(), 1, 1, 0};
    // the reference's failure counter (dwgsim.c:635) runs over the pairs of ONE contig in index order: it is carried from the previous
    // batch only when this one continues it; any other range starts from zero unless the caller supplied the carry (sharded jobs)
    const dwgsim_hip_range_t *r_first = nullptr, *r_last = nullptr;
    for (int q = 0; q < n; ++q) if (r[q].n_pairs) { if (!r_first) r_first = &r[q]; r_last = &r[q]; }
    if (!r_first) { r_first = &r[0]; r_last = &r[n - 1]; }
    const bool continues = c->chain_contig == r_first->contig && c->chain_next_ii == r_first->first_ii && r_first->first_ii != 0;
    const ChainSet ch{c->d_chain.get<uint64_t>(), run.rand_base != DWGSIM_HIP_RAND_CHAIN ? 1 : 0, (c->has_carry_override || !continues) ? 1 : 0, c->has_carry_override ? c->carry_override : 0};
    c->has_carry_override = false; c->chain_contig = r_last->contig; c->chain_next_ii = r_last->first_ii + r_last->n_pairs;
    if (sl.ranges.data() != r) sl.ranges.assign(r, r + n);
    return ch;
}

// The enqueue step: [chain set] -> launch_init -> k_simulate -> abort-rule epilogue -> [k_gzip] -> counters to the slot's pinned mirror -> event
static int sim_launch(dwgsim_hip_ctx_t *c, int slot, Launch &L, const SimPlan &P, const ChainSet &ch, const SimRun &run)
{
    Slot &sl = c->slot[slot]; SimArgs &a = L.a; const SimForm &f = L.f; uint64_t *cnt = sl.counters.dev();
    const uint64_t n_pairs = L.n_pairs, rand_base = run.rand_base; const uint32_t nblk = L.nblk;
    for (int t = 0; t < N_STREAMS; ++t) sl.out_bytes[t] = sl.gz_bytes[t] = 0;
    sl.n_pairs = n_pairs; sl.empty = n_pairs == 0; sl.truth_timed = false;
    if (n_pairs == 0) { if (ch.set_rand || ch.set_carry) launch_chain_set(c->stream.get(), ch.words, rand_base, ch.set_rand, ch.carry, ch.set_carry); return DWGSIM_HIP_OK; }
    uint32_t opens = 0; for (const SimSeg &s : L.segs) opens |= s.contig_start;      // (ranges that begin their contig)
    memcpy(sl.h_segs.get(), L.segs.data(), P.segs);
    HIPC(c, hipMemcpyAsync(sl.segs.get(), sl.h_segs.get(), P.segs, hipMemcpyHostToDevice, c->stream.get()));
    a.segs = sl.segs.get<SimSeg>(); a.n_seg = (int32_t)L.segs.size(); a.n_blocks = nblk; a.n_pairs = n_pairs; a.chain = ch.words; a.lb_shift = P.lb_shift;
    a.meta = c->meta.get<uint32_t>(); a.block_rand = c->block_rand.get<uint32_t>(); a.counters = cnt;
    for (int t = 0; t < 3; ++t) a.out[t] = c->out[slot][t].get<uint8_t>();
    for (int j = 0; j < 4; ++j) a.status[j] = f.split ? nullptr : c->status_all.get<uint64_t>() + (size_t)j * (size_t)nblk;
    if (f.split) { a.split_state = c->split_state.get<uint32_t>(); a.split_hand = c->split_hand.get<uint32_t>(); a.split_agg = c->split_agg.get<uint32_t>(); a.split_pre = c->split_pre.get<uint64_t>(); a.split_chunk = c->split_chunk.get<uint64_t>(); }
    if (P.scratch) { a.flow_scratch = c->flow_scratch.get<uint32_t>(); a.flow_free = c->flow_free.get<uint64_t>(); a.flow_slots = P.flow_slots; }
    sl.group = c->handles[(size_t)L.g->first_handle].group;
    // one operation in front of the kernel: counters, look-back words (the four arrays are contiguous), the scratch slots' free lists, the running values
    launch_init(c->stream.get(), cnt, (uint32_t)N_COUNTERS, a.status[0], f.split ? 0 : 4 * (uint64_t)nblk, a.flow_free, a.flow_free ? 256 + 8 * (uint64_t)nblk : 0,
                ch.words, rand_base, ch.set_rand, ch.carry, ch.set_carry);
    HIPC(c, hipEventRecord(sl.ev_k0.get(), c->stream.get()));
    c->dbg.sim_form = (int64_t)f.nthr << 20 | f.lpp << 16 | f.out << 12 | f.dt << 8 | f.wr << 4 | f.split;
    if (!launch_simulate(c->stream.get(), a, f)) { c->err = "simulate: no k_simulate instance for this form"; return DWGSIM_HIP_ERR_FAILED; }
    HIPC(c, hipEventRecord(sl.ev_k1.get(), c->stream.get()));
    sl.cap_mult = c->flow_cap_mult;
    if (!run.again) launch_failrule(c->stream.get(), a.meta, n_pairs, opens, c->fail_summ.get<uint64_t>(), cnt, c->d_chain.get<uint64_t>());
    // the true read depth: counted by the first run of a batch alone (a second run replays the same ends)
    const bool depth = c->depth_on && !run.again && L.g->depth_valid && !L.g->depth_pos.empty();
    if (P.cap[3] || depth) {
        // The truth step (dw_truth.hpp): this batch's alignments as SAM text, replayed from what the launch left.  It reads meta, which belongs to the CONTEXT, not
        // to the slot -- the next batch's k_simulate overwrites it -- and the slot's FASTQ text and counters: all of it is safe because the step runs on the
        // stream of the launches, behind this batch's kernels and in front of the next batch's (and of the gzip kernels below, which take the SAM as a fourth stream).
        TruthArgs t; memset(&t, 0, sizeof t);
        sl.truth_timed = true;
        HIPC(c, hipEventRecord(sl.ev_t0.get(), c->stream.get()));
        t.lpp = f.lpp; t.bfast = a.p.has_bwa ? 0 : 1; t.prefix_len = c->read_prefix.empty() ? 0 : (int32_t)c->read_prefix.size() + 1; t.qname_max = P.t_qname_max;
        DepthArgs dp; dp.pos = L.g->mem.d_depth_pos.get<int32_t>(); dp.n = (uint32_t)L.g->depth_pos.size(); dp.cnt = L.g->mem.d_depth_cnt.get<unsigned long long>();
        for (int q = 0; P.cap[3] && q < (t.bfast ? 1 : f.lpp); ++q) {
            const int st = t.bfast ? 2 : q;
            t.src[q] = a.out[st]; t.src_bytes[q] = &cnt[text_len_counter(st)]; t.src_cap[q] = P.cap[st];
            t.nl_count[q] = c->t_nl[q].get<uint32_t>(); t.rec[q] = c->t_rec[q].get<uint32_t>(); t.n_rec[q] = t.bfast ? n_pairs * (uint64_t)f.lpp : n_pairs;
        }
        t.ends = c->t_ends.get<TruthEnd>(); t.line_len = c->t_len.get<uint32_t>(); t.blk = c->t_blk.get<uint32_t>();
        t.out = c->out[slot][3].get<uint8_t>(); t.cap = P.cap[3]; t.total = &cnt[text_len_counter(3)];
        t.md = c->truth_md ? 1 : 0; t.ref = L.g->mem.d_ref.get(); t.fit = &cnt[TRUTH_FIT_COUNTER];
        if (P.cap[3]) launch_truth(c->stream.get(), a, t, depth ? &dp : nullptr);
        else launch_truth_depth(c->stream.get(), a, t, dp);
        HIPC(c, hipEventRecord(sl.ev_t1.get(), c->stream.get()));
    }
    if (c->gzip_on) {      // the .gz form of every stream, enqueued behind the text (lengths are read on the device: gz_src_len_counter)
        HIPC(c, hipMemsetAsync(sl.gz_status.get(), 0, P.gz_status, c->stream.get()));
        size_t off = 0;
        for (int t = 0; t < N_STREAMS; ++t) {
            if (P.cap[t] == 0) continue;
            launch_gzip(c->stream.get(), c->out[slot][t].get<uint8_t>(), &cnt[gz_src_len_counter(t, c->truth_md)], P.cap[t], sl.gz_out[t].get<uint8_t>(), P.gz_cap[t], sl.gz_status.get<uint64_t>() + off,
                        &cnt[gz_ticket_counter(t)], &cnt[gz_len_counter(t)], &cnt[STATUS_COUNTER], c->d_crc_table.get<uint32_t>(), c->d_crc_shift.get<uint32_t>());
            off += P.gz_chunks[t];
        }
    }
    HIPC(c, hipEventRecord(sl.ev_end.get(), c->stream.get()));
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(sl.counters.host(), cnt, N_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream.get()));
    HIPC(c, hipEventRecord(sl.ev_done.get(), c->stream.get()));
    sl.pending = true;
    return DWGSIM_HIP_OK;
}

// Enqueue one batch on the compute stream: resolve -> plan -> reserve -> chain -> enqueue.  Every buffer the batch needs is in place before anything
// is enqueued or the chain state moves, so a failing call leaves the context as it found it.
static int sim_enqueue(dwgsim_hip_ctx_t *c, const dwgsim_hip_range_t *r, int n, int slot, const SimRun &run)
{
    if (!c || slot < 0 || slot >= DWGSIM_HIP_SLOTS) { if (c) c->err = "bad simulate arguments"; return DWGSIM_HIP_ERR_ARG; }
    if (c->slot[slot].pending) { c->err = "simulate: the slot still holds a batch that was not waited for"; return DWGSIM_HIP_ERR_STATE; }
    Launch L;
    if (const int rc = sim_resolve(c, r, n, L)) return rc;
    HIPC(c, hipSetDevice(c->device));
    const SimPlan P = sim_plan(c, L, run);
    if (P.too_many) { c->err = "too many pairs in one call"; return DWGSIM_HIP_ERR_ARG; }
    if (L.n_pairs) { if (const int rc = sim_reserve(c, slot, P)) return rc; }
    if (L.n_pairs && c->depth_on && !run.again) { if (const int rc = depth_prepare(c, *L.g)) return rc; }
    // ---- nothing below fails for want of memory ----
    return sim_launch(c, slot, L, P, sim_chain(c, c->slot[slot], r, n, run), run);
}

int dwgsim_hip_simulate_ranges_async(dwgsim_hip_ctx_t *c, const dwgsim_hip_range_t *r, int n, uint64_t rand_base, int slot) { return sim_enqueue(c, r, n, slot, SimRun{rand_base, false, 0}); }

int dwgsim_hip_simulate_async(dwgsim_hip_ctx_t *c, int contig, uint64_t first_ii, uint64_t n_pairs, uint64_t rand_base, int slot)
{
    dwgsim_hip_range_t r; memset(&r, 0, sizeof r); r.contig = contig; r.first_ii = first_ii; r.n_pairs = n_pairs;
    return dwgsim_hip_simulate_ranges_async(c, &r, 1, rand_base, slot);
}

// The waited-for batch of a slot once more, and the wait for it (dwgsim_hip_wait: larger flow buffers, or truth_bytes of room for the truth SAM).  The abort
// rule's epilogue does not run again, so what it left in the block is kept across the run: its segment, verdict and carry, and the chain base the run starts from.
static int sim_rerun(dwgsim_hip_ctx_t *c, int slot, uint64_t truth_bytes)
{
    static const int kept[7] = {fail_seg_counter(0), fail_seg_counter(1), fail_seg_counter(2), fail_seg_counter(3), ABORT_COUNTER, CARRY_COUNTER, CHAIN_BASE_COUNTER};
    Slot &sl = c->slot[slot]; uint64_t *h = sl.counters.host();
    uint64_t keep[7]; for (int q = 0; q < 7; ++q) keep[q] = h[kept[q]];
    if (const int rc = sim_enqueue(c, sl.ranges.data(), (int)sl.ranges.size(), slot, SimRun{h[CHAIN_BASE_COUNTER], true, truth_bytes})) return rc;
    HIPC(c, hipEventSynchronize(sl.ev_done.get())); sl.pending = false;
    for (int q = 0; q < 7; ++q) h[kept[q]] = keep[q];
    return DWGSIM_HIP_OK;
}

// What the counter block of a finished batch says: DWGSIM_HIP_OK, or the error and its message.  Blame goes in this order; a bit that is none of the later rungs' counts as used-up attempts.
static int batch_verdict(dwgsim_hip_ctx_t *c, const uint64_t *h)
{
    const uint64_t st = h[STATUS_COUNTER];
    if (st & REGIONS_BIT) { c->err = "dwgsim-hip: no fragment placement satisfied the target regions (-x) after 2^20 tries (the reference would not terminate)\n"; return DWGSIM_HIP_ERR_FAILED; }
    if (st & FLOW_ROOM_BIT) { c->err = "dwgsim-hip: a read outgrew its buffer (or degenerated) in the flow-error model\n"; return DWGSIM_HIP_ERR_FAILED; }
    if ((st & ~(GZIP_ROOM_BIT | TRUTH_ERR_BIT | TRUTH_ROOM_BIT)) || h[ABORT_COUNTER]) return fail_attempts(c);
    if (st & GZIP_ROOM_BIT) { c->err = "dwgsim-hip: the gzip output buffer is too small for this text\n"; return DWGSIM_HIP_ERR_FAILED; }
    if (st & TRUTH_ERR_BIT) { c->err = "dwgsim-hip: the truth SAM could not be made (a read's record or alignment could not be replayed)\n"; return DWGSIM_HIP_ERR_FAILED; }
    if (st & TRUTH_ROOM_BIT) { c->err = "dwgsim-hip: the truth SAM did not fit its buffer\n"; return DWGSIM_HIP_ERR_FAILED; }
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_wait(dwgsim_hip_ctx_t *c, int slot, dwgsim_hip_batch_t *out)
{
    if (!c || slot < 0 || slot >= DWGSIM_HIP_SLOTS) { if (c) c->err = "bad slot"; return DWGSIM_HIP_ERR_ARG; }
    Slot &sl = c->slot[slot];
    if (out) memset(out, 0, sizeof *out);
    if (sl.empty) { sl.pending = false; return DWGSIM_HIP_OK; }
    if (!sl.pending) { c->err = "wait: no batch was enqueued on this slot"; return DWGSIM_HIP_ERR_STATE; }
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipEventSynchronize(sl.ev_done.get()));
    sl.pending = false;
    const uint64_t *h = sl.counters.host();
    if ((h[STATUS_COUNTER] & FLOW_ROOM_BIT) && !(h[STATUS_COUNTER] & ~(FLOW_ROOM_BIT | GZIP_ROOM_BIT)) && c->prm.data_type == 2) {
        // a read outgrew its flow-space buffers: the reference doubles them and goes on, without end (dwgsim.c:296-311); here the batch runs again with twice
        // the capacity (kept for the rest of the job), up to FLOW_CAP_MAX bases per read -- two thousand times a 400-base read, in scratch slots whose number
        // shrinks as they grow (sim_plan; the retired 16 x limit: DESIGN.md §4, Ion Torrent)
        while (h[STATUS_COUNTER] & FLOW_ROOM_BIT) {
            if (sl.cap_mult >= c->flow_cap_mult) {      // (another batch may have doubled it already)
                if ((int64_t)flow_base_capacity(c) * (int64_t)c->flow_cap_mult * 2 > (int64_t)FLOW_CAP_MAX) break;
                c->flow_cap_mult *= 2;
            }
            if (const int rc = sim_rerun(c, slot, 0)) return rc;
        }
    }
    if (h[STATUS_COUNTER] == TRUTH_ROOM_BIT && !h[ABORT_COUNTER]) {      // (nothing else went wrong: the first run's gzip took none of the SAM, TruthArgs::fit)
        // The tagged truth SAM did not fit its planned buffer (sim_plan: MD has no bound in the read length).  The scan left the exact size in its counter, so the
        // batch runs once more with that much room.  Record and line offsets are 32-bit words: a batch whose SAM would pass 4 GiB is refused.
        const uint64_t need = h[text_len_counter(3)];
        if (need + 64 >= (1ull << 32)) { c->err = "dwgsim-hip: the truth SAM of one batch would pass 4 GiB with its MD strings (deletions are spelled out): use smaller batches\n"; return DWGSIM_HIP_ERR_UNSUP; }
        if (const int rc = sim_rerun(c, slot, need)) return rc;
        ++c->dbg.truth_reruns;
        if (h[STATUS_COUNTER] & TRUTH_ROOM_BIT) { c->err = "dwgsim-hip: the truth SAM did not fit the room its own scan asked for\n"; return DWGSIM_HIP_ERR_FAILED; }
    }
    if (const int rc = batch_verdict(c, h)) return rc;
    for (int t = 0; t < N_STREAMS; ++t) { sl.out_bytes[t] = h[text_len_counter(t)]; sl.gz_bytes[t] = h[gz_len_counter(t)]; }
    if (!c->truth_on) sl.out_bytes[3] = sl.gz_bytes[3] = 0;
    if (c->dbg.phases) {   // only meaningful with the -DDW_PHASE_TIMING build (tools/phase_profile.sh)
        uint64_t tot = 0; for (int k = 0; k < N_PHASES; ++k) tot += h[phase_counter(k)];
        fprintf(stderr, "[phases]");
        for (int k = 0; k < N_PHASES; ++k) fprintf(stderr, " p%d=%.1f%%", k, tot ? 100.0 * h[phase_counter(k)] / tot : 0.0);
        fprintf(stderr, " (ticks %llu)\n", (unsigned long long)tot);
    }
    if (out) {
        out->n_pairs = sl.n_pairs; out->n_random = h[RANDOM_COUNTER]; out->n_retries = h[RETRY_COUNTER];
        for (int t = 0; t < 3; ++t) { out->bytes[t] = sl.out_bytes[t]; out->gz_bytes[t] = sl.gz_bytes[t]; out->dev_ptr[t] = c->out[slot][t].get(); }
        if (sl.truth_timed) { float ms = 0; HIPC(c, hipEventElapsedTime(&ms, sl.ev_t0.get(), sl.ev_t1.get())); c->dbg.truth_us = 1e3 * ms; }
        out->sam_bytes = sl.out_bytes[3]; out->sam_gz_bytes = sl.gz_bytes[3]; out->sam_dev_ptr = sl.out_bytes[3] ? c->out[slot][3].get() : nullptr;
        for (int t = 0; t < 4; ++t) out->fail_seg[t] = h[fail_seg_counter(t)];
        out->fail_carry = h[CARRY_COUNTER];
        HIPC(c, hipEventElapsedTime(&out->sim_kernel_ms, sl.ev_k0.get(), sl.ev_k1.get()));
        HIPC(c, hipEventElapsedTime(&out->kernel_ms, sl.ev_k0.get(), sl.ev_end.get()));       // ... with the abort-rule epilogue and the gzip kernels
    }
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_simulate(dwgsim_hip_ctx_t *c, int contig, uint64_t first_ii, uint64_t n_pairs, uint64_t rand_base, int slot, dwgsim_hip_batch_t *out)
{
    if (out) memset(out, 0, sizeof *out);
    const int rc = dwgsim_hip_simulate_async(c, contig, first_ii, n_pairs, rand_base, slot);
    if (rc != DWGSIM_HIP_OK) return rc;
    return dwgsim_hip_wait(c, slot, out);
}

// Page-locked host memory: anonymous memory on TRANSPARENT HUGE PAGES, touched by the calling thread(s) (so it lies on their NUMA node) and then registered
// with the runtime.  Page-locking is paid per page: hipHostMalloc locks 4 KB pages at 5-6 GB/s -- 60-85 ms for the 300 MB staging of a chromosome, on
// the critical path of a job's first batch, and the KFD's per-process lock makes every other allocation of the process wait meanwhile -- while 2 MB
// pages register at 17-55 GB/s (tools/ubench_pin.hip, profiles/r05_genome_trace.txt); copies into either run at the same 49-50 GB/s.  Where the kernel
// grants no huge pages (transparent_hugepage = never) the same code simply registers 4 KB pages.
namespace {
struct HostRegion { uint8_t *base; size_t len; };
std::mutex g_host_m;
std::vector<HostRegion> g_host;      // (a handful per process)
}
static bool in_host_registry(const void *p)
{
    std::lock_guard<std::mutex> lk(g_host_m);
    for (const HostRegion &r : g_host) if ((const uint8_t *)p >= r.base && (const uint8_t *)p < r.base + r.len) return true;
    return false;
}
void *dwgsim_hip_host_alloc(size_t bytes)
{
    const size_t H = (size_t)2 << 20;
    const size_t len = ((bytes ? bytes : 1) + H - 1) / H * H;
    uint8_t *raw = (uint8_t *)mmap(nullptr, len + H, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (raw == MAP_FAILED) return nullptr;
    uint8_t *p = (uint8_t *)(((uintptr_t)raw + H - 1) & ~(uintptr_t)(H - 1));
    if (p > raw) munmap(raw, (size_t)(p - raw));
    if (p + len < raw + len + H) munmap(p + len, (size_t)(raw + len + H - (p + len)));
    (void)madvise(p, len, MADV_HUGEPAGE);
    // first touch (a fault per huge page zeroes 2 MB): large buffers by a few threads at once
    auto touch = [p](size_t from, size_t upto) { for (size_t o = from; o < upto; o += 4096) ((volatile uint8_t *)p)[o] = 0; };
    const int nt = len >= ((size_t)64 << 20) ? 4 : 1;
    if (nt == 1) touch(0, len);
    else {
        std::vector<std::thread> th; const size_t per = (len / H + (size_t)nt - 1) / (size_t)nt * H;
        for (int k = 0; k < nt; ++k) { const size_t a = std::min(len, (size_t)k * per), b = std::min(len, a + per); if (b > a) th.emplace_back(touch, a, b); }
        for (auto &t : th) t.join();
    }
    if (hipHostRegister(p, len, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); munmap(p, len); return nullptr; }
    { std::lock_guard<std::mutex> lk(g_host_m); g_host.push_back(HostRegion{p, len}); }
    return p;
}
void dwgsim_hip_host_free(void *p)
{
    if (!p) return;
    HostRegion r{nullptr, 0};
    {
        std::lock_guard<std::mutex> lk(g_host_m);
        for (size_t i = 0; i < g_host.size(); ++i) if (g_host[i].base == (uint8_t *)p) { r = g_host[i]; g_host.erase(g_host.begin() + (long)i); break; }
    }
    if (!r.base) return;      // (not one of ours)
    (void)hipHostUnregister(r.base);
    munmap(r.base, r.len);
}

static bool is_slot_stream(const dwgsim_hip_ctx_t *c, int slot, int stream) { return c && slot >= 0 && slot < DWGSIM_HIP_SLOTS && stream >= 0 && stream < N_STREAMS && (stream != DWGSIM_HIP_STREAM_SAM || c->truth_on); }      // (no SAM stream while the truth SAM is off)
// Copies on the context's second stream: a batch that is being copied out of one slot overlaps with the kernels filling the other.  gz: the
// stream's gzip members instead of its text.
static int fetch_async(dwgsim_hip_ctx_t *c, int slot, int stream, void *host_dst, size_t cap, bool gz)
{
    if (!is_slot_stream(c, slot, stream) || (!host_dst && cap)) { if (c) c->err = "bad fetch arguments"; return DWGSIM_HIP_ERR_ARG; }
    Slot &sl = c->slot[slot];
    if (sl.pending) { c->err = "fetch: wait for the batch first (its sizes are not known yet)"; return DWGSIM_HIP_ERR_STATE; }
    HIPC(c, hipSetDevice(c->device));
    const size_t n = (size_t)(gz ? sl.gz_bytes[stream] : sl.out_bytes[stream]);
    if (n > cap) { c->err = "fetch: destination too small"; return DWGSIM_HIP_ERR_ARG; }
    if (n == 0) return DWGSIM_HIP_OK;
    HIPC(c, hipMemcpyAsync(host_dst, gz ? sl.gz_out[stream].get() : c->out[slot][stream].get(), n, hipMemcpyDeviceToHost, c->copy_stream.get()));
    HIPC(c, hipEventRecord(sl.ev_fetched.get(), c->copy_stream.get()));
    sl.fetch_in_flight = true;
    return DWGSIM_HIP_OK;
}
int dwgsim_hip_fetch_async(dwgsim_hip_ctx_t *c, int slot, int stream, void *host_dst, size_t cap) { return fetch_async(c, slot, stream, host_dst, cap, false); }

int dwgsim_hip_set_gzip(dwgsim_hip_ctx_t *c, int on)
{
    if (!c) return DWGSIM_HIP_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    if (on && !c->d_crc_shift) {      // (d_crc_shift is made last: both tables are there when it is)
        std::vector<uint32_t> tab(4 * 256), sh(16 * 1024);
        gz_host_tables(tab.data(), sh.data());
        if (upload(c, c->d_crc_table, tab.data(), tab.size() * 4) || upload(c, c->d_crc_shift, sh.data(), sh.size() * 4)) return DWGSIM_HIP_ERR_DEVICE;
    }
    c->gzip_on = on != 0;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_fetch_gz_async(dwgsim_hip_ctx_t *c, int slot, int stream, void *host_dst, size_t cap) { return fetch_async(c, slot, stream, host_dst, cap, true); }

// The truth SAM (DESIGN.md "6e").  Switched on, every simulate call also leaves stream DWGSIM_HIP_STREAM_SAM; switched off nothing of it is launched or allocated.
int dwgsim_hip_set_truth_sam(dwgsim_hip_ctx_t *c, int on)
{
    if (!c) return DWGSIM_HIP_ERR_ARG;
    for (const Slot &sl : c->slot) if (sl.pending) { c->err = "set_truth_sam: a batch is in flight (wait for every slot first)"; return DWGSIM_HIP_ERR_STATE; }
    if (on && c->prm.data_type != 0) {
        c->err = c->prm.data_type == 1 ? "dwgsim-hip: no truth SAM for SOLiD reads (-c 1): colour space has no base-space SEQ\n"
                                       : "dwgsim-hip: no truth SAM for Ion Torrent reads (-c 2): the flow model adds indels of its own that a haplotype CIGAR would not show\n";
        return DWGSIM_HIP_ERR_UNSUP;
    }
    if (on) { HIPC(c, hipSetDevice(c->device)); for (Slot &sl : c->slot) { HIPC(c, sl.ev_t0.create()); HIPC(c, sl.ev_t1.create()); } }
    c->truth_on = on != 0;
    return DWGSIM_HIP_OK;
}
// ... with NM:i: and MD:Z: on every mapped record (DESIGN.md "6e", the law: dw_truth.hpp).  A switch on top of the truth SAM: while that is off it does nothing.
int dwgsim_hip_set_truth_md(dwgsim_hip_ctx_t *c, int on)
{
    if (!c) return DWGSIM_HIP_ERR_ARG;
    for (const Slot &sl : c->slot) if (sl.pending) { c->err = "set_truth_md: a batch is in flight (wait for every slot first)"; return DWGSIM_HIP_ERR_STATE; }
    if (on && c->prm.data_type != 0) { c->err = "dwgsim-hip: no truth SAM, and so no NM / MD tags, for SOLiD and Ion Torrent reads (-c 1, -c 2)\n"; return DWGSIM_HIP_ERR_UNSUP; }
    c->truth_md = on != 0;
    return DWGSIM_HIP_OK;
}

// The true read depth of every listed mutated cell (DESIGN.md "6f"; the rule: dw_truth.hpp k_truth_depth).  Switched on, every batch adds to the counters of its
// group, with or without the truth SAM; switched off nothing of it is launched or allocated.
int dwgsim_hip_set_truth_depth(dwgsim_hip_ctx_t *c, int on)
{
    if (!c) return DWGSIM_HIP_ERR_ARG;
    for (const Slot &sl : c->slot) if (sl.pending) { c->err = "set_truth_depth: a batch is in flight (wait for every slot first)"; return DWGSIM_HIP_ERR_STATE; }
    if (on && c->prm.data_type != 0) {
        c->err = c->prm.data_type == 1 ? "dwgsim-hip: no true read depth for SOLiD reads (-c 1): it is counted from the alignments of the truth SAM, which colour space does not have\n"
                                       : "dwgsim-hip: no true read depth for Ion Torrent reads (-c 2): it is counted from the alignments of the truth SAM, which the flow model's own indels rule out\n";
        return DWGSIM_HIP_ERR_UNSUP;
    }
    if (on) { HIPC(c, hipSetDevice(c->device)); for (Slot &sl : c->slot) { HIPC(c, sl.ev_t0.create()); HIPC(c, sl.ev_t1.create()); } }
    c->depth_on = on != 0;
    return DWGSIM_HIP_OK;
}
// The counters of one contig: its slice of the group's list, in list order, two per cell (haplotype 1, haplotype 2) -- everything this context has simulated
// for it since its walk.  Waits for the batches the context has enqueued.  Returns the cells of the slice; at most cap_cells of them are written.
int64_t dwgsim_hip_truth_depth_fetch(dwgsim_hip_ctx_t *c, int contig, uint64_t *counts, size_t cap_cells)
{
    int km = 0;
    Group *gp = c ? get_group(c, contig, &km) : nullptr;
    if (!gp) return DWGSIM_HIP_ERR_ARG;
    if (!c->depth_on) { c->err = "truth_depth_fetch: the true read depth is switched off (dwgsim_hip_set_truth_depth)"; return DWGSIM_HIP_ERR_ARG; }
    if (!counts && cap_cells) { c->err = "bad truth_depth_fetch arguments"; return DWGSIM_HIP_ERR_ARG; }
    Group &g = *gp;
    if (!g.mutated || g.walk_pending) { c->err = "mutate_contig must run first"; return DWGSIM_HIP_ERR_STATE; }
    HIPC(c, hipSetDevice(c->device));
    if (const int rc = depth_prepare(c, g)) return rc;      // (no batch yet: zeroes)
    const Member &m = g.m[(size_t)km];
    const auto b = g.depth_pos.begin(), e = g.depth_pos.end();
    const size_t e0 = (size_t)(std::lower_bound(b, e, m.start) - b), e1 = (size_t)(std::lower_bound(b, e, (int32_t)(m.start + m.l)) - b);
    const size_t n = e1 - e0, take = n < cap_cells ? n : cap_cells;
    if (take) HIPC(c, hipMemcpyAsync(counts, g.mem.d_depth_cnt.get<uint64_t>() + 2 * e0, 2 * sizeof(uint64_t) * take, hipMemcpyDeviceToHost, c->stream.get()));      // (behind the batches)
    HIPC(c, hipStreamSynchronize(c->stream.get()));
    return (int64_t)n;
}

// The header of a truth VCF: that of mutations.vcf with the three FORMAT lines in front of #CHROM and the sample column behind it.  Host text, one function for
// every caller, with the calling rules of dwgsim_hip_truth_sam_header.
int64_t dwgsim_hip_truth_vcf_header(const char *const *names, const int64_t *lens, int n, char *buf, size_t cap)
{
    if (n < 0 || (n > 0 && (!names || !lens)) || (!buf && cap)) return DWGSIM_HIP_ERR_ARG;
    std::string h = "##fileformat=VCFv4.1\n";
    for (int k = 0; k < n; ++k) { if (!names[k]) return DWGSIM_HIP_ERR_ARG; h += "##contig=<ID="; h += names[k]; h += ",length=" + std::to_string((int)lens[k]) + ">\n"; }
    h += "##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele Frequency\">\n"
         "##INFO=<ID=pl,Number=1,Type=Integer,Description=\"Phasing: 1 - HET contig 1, #2 - HET contig #2, 3 - HOM both contigs\">\n"
         "##INFO=<ID=mt,Number=1,Type=String,Description=\"Variant Type: SUBSTITUTE/INSERT/DELETE\">\n"
         "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype, phased: haplotype 1 | haplotype 2\">\n"
         "##FORMAT=<ID=AD,Number=.,Type=Integer,Description=\"Simulated read ends that hold the site, by the haplotype they were read from: ref,alt\">\n"
         "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Simulated read ends that hold the site, both haplotypes\">\n"
         "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tdwgsim\n";
    if (buf) memcpy(buf, h.data(), h.size() < cap ? h.size() : cap);
    return (int64_t)h.size();
}

// The header of a truth SAM: host text, the same bytes for every caller.  One @SQ per contig of the table, in its order.  Returns the bytes the header has
// (whatever cap is); at most cap of them are written to buf (may be NULL with cap 0: the size alone).
int64_t dwgsim_hip_truth_sam_header(const char *const *names, const int64_t *lens, int n, char *buf, size_t cap)
{
    if (n < 0 || (n > 0 && (!names || !lens)) || (!buf && cap)) return DWGSIM_HIP_ERR_ARG;
    std::string h = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
    for (int k = 0; k < n; ++k) { if (!names[k]) return DWGSIM_HIP_ERR_ARG; h += "@SQ\tSN:"; h += names[k]; h += "\tLN:" + std::to_string((long long)lens[k]) + "\n"; }
    h += "@PG\tID:dwgsim-hip\tPN:dwgsim-hip\tDS:true alignments of the simulated reads\n";
    if (buf) memcpy(buf, h.data(), h.size() < cap ? h.size() : cap);
    return (int64_t)h.size();
}

int dwgsim_hip_fetch_wait(dwgsim_hip_ctx_t *c, int slot)
{
    if (!c || slot < 0 || slot >= DWGSIM_HIP_SLOTS) { if (c) c->err = "bad slot"; return DWGSIM_HIP_ERR_ARG; }
    Slot &sl = c->slot[slot];
    if (!sl.fetch_in_flight) return DWGSIM_HIP_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipEventSynchronize(sl.ev_fetched.get()));
    sl.fetch_in_flight = false;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_fetch(dwgsim_hip_ctx_t *c, int slot, int stream, void *host_dst, size_t cap)
{
    if (!is_slot_stream(c, slot, stream) || (!host_dst && cap)) return DWGSIM_HIP_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    Slot &sl = c->slot[slot];
    if (sl.pending) { c->err = "fetch: wait for the batch first (its sizes are not known yet)"; return DWGSIM_HIP_ERR_STATE; }
    const size_t n = (size_t)sl.out_bytes[stream];
    if (n > cap) { c->err = "fetch: destination too small"; return DWGSIM_HIP_ERR_ARG; }
    if (n == 0) return DWGSIM_HIP_OK;
    if (is_page_locked(host_dst)) {   // a pinned (page-locked / registered) destination takes one direct copy at link speed
        HIPC(c, hipMemcpyAsync(host_dst, c->out[slot][stream].get(), n, hipMemcpyDeviceToHost, c->copy_stream.get()));
        HIPC(c, hipStreamSynchronize(c->copy_stream.get()));
        return DWGSIM_HIP_OK;
    }
    // double-buffered pinned staging: D2H of chunk k+1 overlaps the host copy of chunk k
    const size_t CH = (size_t)16 << 20;
    HIPC(c, c->h_stage.reserve(2 * CH, 2 * CH));
    const uint8_t *src = c->out[slot][stream].get<uint8_t>();
    uint8_t *stage[2] = {c->h_stage.get<uint8_t>(), c->h_stage.get<uint8_t>() + CH};
    size_t done = 0; int b = 0;
    size_t cur = n < CH ? n : CH;
    HIPC(c, hipMemcpyAsync(stage[0], src, cur, hipMemcpyDeviceToHost, c->copy_stream.get()));
    while (done < n) {
        HIPC(c, hipStreamSynchronize(c->copy_stream.get()));
        const size_t next_off = done + cur, next = next_off < n ? ((n - next_off) < CH ? (n - next_off) : CH) : 0;
        if (next) HIPC(c, hipMemcpyAsync(stage[b ^ 1], src + next_off, next, hipMemcpyDeviceToHost, c->copy_stream.get()));
        memcpy((uint8_t *)host_dst + done, stage[b], cur);
        done += cur; cur = next; b ^= 1;
    }
    return DWGSIM_HIP_OK;
}

// Test / analysis hook (not part of the drop-in surface): occurrences of `byte` in one finished stream of a waited-for slot, counted on the device.
int dwgsim_hip_debug_count_byte(dwgsim_hip_ctx_t *c, int slot, int stream, int byte, uint64_t *count)
{
    if (!is_slot_stream(c, slot, stream) || !count) return DWGSIM_HIP_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    Slot &sl = c->slot[slot];
    if (sl.pending) { c->err = "count_byte: wait for the batch first"; return DWGSIM_HIP_ERR_STATE; }
    HIPC(c, hipMemsetAsync(&c->counters.dev()[COUNT_BYTE_COUNTER], 0, sizeof(uint64_t), c->stream.get()));
    if (sl.out_bytes[stream]) launch_count_byte(c->stream.get(), c->out[slot][stream].get<uint8_t>(), sl.out_bytes[stream], (uint32_t)(byte & 0xff), &c->counters.dev()[COUNT_BYTE_COUNTER]);
    HIPC(c, hipMemcpyAsync(&c->counters.host()[COUNT_BYTE_COUNTER], &c->counters.dev()[COUNT_BYTE_COUNTER], sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream.get()));
    HIPC(c, hipStreamSynchronize(c->stream.get()));
    *count = c->counters.host()[COUNT_BYTE_COUNTER];
    return DWGSIM_HIP_OK;
}

// Test hook (not part of the drop-in surface): the gzip kernel on arbitrary host bytes (the product only ever feeds it FASTQ text): the members
// of `n` bytes of `text` into `out` (cap bytes), *out_n = their total size.  Synchronous.
int dwgsim_hip_debug_gzip(dwgsim_hip_ctx_t *c, const void *text, size_t n, void *out, size_t cap, size_t *out_n)
{
    if (!c || (!text && n) || !out_n) return DWGSIM_HIP_ERR_ARG;
    HIPC(c, hipSetDevice(c->device));
    if (const int rc = dwgsim_hip_set_gzip(c, c->gzip_on ? 1 : 0); rc < 0) return rc;
    if (!c->d_crc_shift) { const bool was = c->gzip_on; if (const int rc = dwgsim_hip_set_gzip(c, 1); rc < 0) return rc; c->gzip_on = was; }
    *out_n = 0;
    if (n == 0) return DWGSIM_HIP_OK;
    const size_t gcap = (size_t)gz_capacity(n), nch = (size_t)gz_chunks(n);
    DevMem text_m, out_m, aux_m;
    if (reserve(c, text_m, n + 64, n + 64) != hipSuccess || reserve(c, out_m, gcap + 64, gcap + 64) != hipSuccess || reserve(c, aux_m, sizeof(uint64_t) * (4 + nch), sizeof(uint64_t) * (4 + nch)) != hipSuccess) { c->err = "out of device memory"; return DWGSIM_HIP_ERR_DEVICE; }
    uint8_t *d_text = text_m.get(), *d_out = out_m.get(); uint64_t *d_aux = aux_m.get<uint64_t>();       // aux: [0] length, [1] ticket, [2] total, [3] flags, [4..] look-back words
    const uint64_t n64 = n;
    bool ok = hipMemcpyAsync(d_text, text, n, hipMemcpyHostToDevice, c->stream.get()) == hipSuccess && hipMemsetAsync(d_aux, 0, sizeof(uint64_t) * (4 + nch), c->stream.get()) == hipSuccess &&
              hipMemcpyAsync(d_aux, &n64, sizeof n64, hipMemcpyHostToDevice, c->stream.get()) == hipSuccess;
    if (ok) {
        launch_gzip(c->stream.get(), d_text, &d_aux[0], n, d_out, gcap, &d_aux[4], &d_aux[1], &d_aux[2], &d_aux[3], c->d_crc_table.get<uint32_t>(), c->d_crc_shift.get<uint32_t>());
        uint64_t res[4] = {0, 0, 0, 0};
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(res, d_aux, sizeof res, hipMemcpyDeviceToHost, c->stream.get()) == hipSuccess && hipStreamSynchronize(c->stream.get()) == hipSuccess;
        if (ok && (res[3] & GZIP_ROOM_BIT)) { c->err = "dwgsim-hip: the gzip output buffer is too small for this text\n"; return DWGSIM_HIP_ERR_FAILED; }
        if (ok && res[2] > cap) { c->err = "debug_gzip: destination too small"; return DWGSIM_HIP_ERR_ARG; }
        if (ok) { ok = hipMemcpy(out, d_out, (size_t)res[2], hipMemcpyDeviceToHost) == hipSuccess; *out_n = (size_t)res[2]; }
    }
    if (!ok) { c->err = "debug_gzip: device error"; return DWGSIM_HIP_ERR_DEVICE; }
    return DWGSIM_HIP_OK;
}

// Test / analysis hooks (not part of the drop-in surface): "justify_seq" = 1 runs the left-justification from one thread (cross-check),
// "walk_cap" = n starts the mutation walk with a capacity of n candidates and a 1-byte inserted-base pool (exercises the exact re-run),
// "phases" = 1 prints the phase split of the -DDW_PHASE_TIMING analysis build,
// "writer" = 0 / 1 forces the register / FIFO record writer of the Illumina kernels (-1: chosen by LDS occupancy),
// "sim_threads" = 64 forces the one-wave blocks of the long-read variant (measured: 25 % slower on 2 x 150 bp, small jobs included),
// "walk_seg_min" = n runs the walk's two serial scans in their segmented form from a capacity of n candidates on (default 16384; 0 restores it),
// "place_cap" = n gives the lists of pairs that k_place leaves open room for n entries each (exercises the second, full-size run),
// "split" = 0 / 1 runs the Illumina read kernel as one kernel with look-backs / as two kernels with the offsets computed in between (-1: two for reads of
// up to 100 bases),
// "qrows" = 0 keeps the quality line of the single Illumina kernel on the per-lane FIFO where it would run in the wave's staging rows (reads of 137 bases on).
int dwgsim_hip_debug_option(dwgsim_hip_ctx_t *c, const char *key, int64_t value)
{
    if (!c || !key) return DWGSIM_HIP_ERR_ARG;
    if (!strcmp(key, "justify_seq")) c->dbg.seq_justify = value != 0;
    else if (!strcmp(key, "dense_view")) c->dbg.dense_view = value != 0;
    else if (!strcmp(key, "walk_cap")) c->dbg.walk_cap = value;
    else if (!strcmp(key, "site_slots")) c->dbg.site_slots = (int)value;
    else if (!strcmp(key, "site_slot_cap")) c->dbg.site_slot_cap = value;
    else if (!strcmp(key, "phases")) c->dbg.phases = value != 0;
    else if (!strcmp(key, "writer")) c->dbg.writer = (int)value;
    else if (!strcmp(key, "sim_threads")) c->dbg.force_threads = (int)value;
    else if (!strcmp(key, "walk_seg_min")) walk_debug_seg_min((uint32_t)value);      // (process-wide)
    else if (!strcmp(key, "place_cap")) c->dbg.place_cap = value;
    else if (!strcmp(key, "truth_cap")) c->dbg.truth_cap = value;      // the bytes a batch's tagged truth SAM is planned with at first (tests: exercises the second run; -1: the product's plan)
    else if (!strcmp(key, "split")) c->dbg.split = (int)value;
    else if (!strcmp(key, "qrows")) c->dbg.qrows = (int)value;
    else if (!strcmp(key, "flow_slots")) c->dbg.flow_slots = (int)value;
    else if (!strcmp(key, "ion_lds")) c->dbg.ion_lds = (int)value;
    else if (!strcmp(key, "flow_cap")) c->dbg.flow_cap_forced = (int)value;
    else if (!strcmp(key, "hap_yardstick")) c->dbg.hap_yardstick = value != 0;      // dwgsim_hip_haplotype_fasta also times a device-to-device copy of the text's size ("hap_copy_us")
    else if (!strcmp(key, "truth_yardstick")) {      // a device-to-device copy of `value` bytes of slot 0's truth SAM, timed at once on the compute stream: debug_get("truth_copy_us")
        Slot &sl = c->slot[0];
        if (!c->truth_on || sl.pending || value <= 0 || (uint64_t)value > sl.out_bytes[3]) { c->err = "truth_yardstick: slot 0 holds no truth SAM of that size"; return DWGSIM_HIP_ERR_ARG; }
        HIPC(c, hipSetDevice(c->device));
        DevMem tmp;
        HIPC(c, reserve(c, tmp, (size_t)value, (size_t)value));
        HIPC(c, hipEventRecord(sl.ev_t0.get(), c->stream.get()));
        HIPC(c, hipMemcpyAsync(tmp.get(), c->out[0][3].get(), (size_t)value, hipMemcpyDeviceToDevice, c->stream.get()));
        HIPC(c, hipEventRecord(sl.ev_t1.get(), c->stream.get()));
        HIPC(c, hipStreamSynchronize(c->stream.get()));
        float ms = 0; HIPC(c, hipEventElapsedTime(&ms, sl.ev_t0.get(), sl.ev_t1.get()));
        c->dbg.truth_copy_us = 1e3 * ms;
    }
    else { c->err = "unknown debug option"; return DWGSIM_HIP_ERR_ARG; }
    return DWGSIM_HIP_OK;
}

// ... and values to read back: "place_open" = pairs the last dwgsim_hip_count_random* call could not settle from the coarse summaries;
// "walk_us" / "count_us" = accumulated HIP-event time (microseconds) of the walk chains / random-read counts of this context
// "sim_form" = the k_simulate form of the last simulate launch (0 before the first): NTHR << 20 | LPP << 16 | OUT << 12 | DT << 8 | WR << 4 | SPLIT,
// where SPLIT = 1 is the two-kernel form and WR the writer of its second half
// "walk_form" = what the last mutation walk enqueued was made of (0 before the first): ATTEMPT << 16 | FILE << 12 | SLOTS << 8 | RESTORE << 4 | DENSE -- the
// attempt (0; 1, 2: the exact re-runs of dwgsim_hip_mutate_wait), FILE 1 the file-driven walk (-m / -b / -v) / 0 the random one, SLOTS 1 the slot form of the
// site scan / 0 the look-back form (and the file-driven walk, which scans no sites), RESTORE what was put back to the pristine copies first (0 nothing, 1 the
// dirty chunks, 2 whole buffers), DENSE 1 the views made from every cell / 0 from the dirty bitmap
int dwgsim_hip_debug_get(dwgsim_hip_ctx_t *c, const char *key, int64_t *value)
{
    if (!c || !key || !value) return DWGSIM_HIP_ERR_ARG;
    if (!strcmp(key, "place_open")) *value = (int64_t)c->dbg.place_open;
    else if (!strcmp(key, "flow_cap_mult")) *value = (int64_t)c->flow_cap_mult;
    else if (!strcmp(key, "walk_us")) *value = (int64_t)c->dbg.walk_us;           // HIP-event time of the walk chains waited for so far (start of the chain to its end, on the walk stream)
    else if (!strcmp(key, "count_us")) *value = (int64_t)c->dbg.count_us;         // ... of the random-read counts (k_place .. k_range_counts)
    else if (!strcmp(key, "sim_form")) *value = c->dbg.sim_form;                  // k_simulate<LPP, OUT, DT, NTHR, WR, SPLIT> of the last launch, packed
    else if (!strcmp(key, "hap_len_us")) *value = (int64_t)c->dbg.hap_len_us;     // the haplotype text built last: HIP-event time of its length pass + scan,
    else if (!strcmp(key, "hap_write_us")) *value = (int64_t)c->dbg.hap_write_us; // ... of its header and write kernels,
    else if (!strcmp(key, "hap_copy_us")) *value = (int64_t)c->dbg.hap_copy_us;   // ... and ("hap_yardstick") of a device-to-device copy of its size
    else if (!strcmp(key, "chain_count_us")) *value = (int64_t)c->dbg.chain_count_us;      // the haplotype chain built last (dwgsim_hip_haplotype_chain): HIP-event time of its count pass + scan,
    else if (!strcmp(key, "chain_write_us")) *value = (int64_t)c->dbg.chain_write_us;      // ... of its write pass,
    else if (!strcmp(key, "chain_blocks")) *value = c->dbg.chain_blocks;                   // ... and the blocks it found
    else if (!strcmp(key, "truth_us")) *value = (int64_t)c->dbg.truth_us;         // HIP-event time (microseconds) of the truth step of the batch waited for last (dwgsim_hip_set_truth_sam)
    else if (!strcmp(key, "truth_reruns")) *value = c->dbg.truth_reruns;         // batches of this context that ran a second time because their tagged truth SAM needed room (dwgsim_hip_set_truth_md)
    else if (!strcmp(key, "truth_copy_us")) *value = (int64_t)c->dbg.truth_copy_us;      // ... and of the copy the option "truth_yardstick" made
    else if (!strcmp(key, "walk_form")) *value = c->dbg.walk_form;                // attempt, file-driven / random, site-scan form, restore, views of the last walk, packed
    else { c->err = "unknown debug value"; return DWGSIM_HIP_ERR_ARG; }
    return DWGSIM_HIP_OK;
}

// ... and the k_simulate<LPP, OUT, DT, NTHR, WR, SPLIT> instances the library was built with (dw_simulate.hip DW_SIM_ALL, the list launch_simulate looks a
// form up in): their number; out (may be NULL) gets at most cap of them, packed as "sim_form" above with SPLIT the template parameter -- 0 the single
// kernel, 1 / 2 the first / second half of the two-kernel form.  Needs no context and no device.
int dwgsim_hip_debug_sim_instances(int64_t *out, int cap)
{
    return sim_instances(out, cap);
}

} // extern "C"
