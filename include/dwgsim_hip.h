/*
 * dwgsim_hip.h -- C-ABI of the MI355X-native dwgsim hot path (libdwgsim_hip.so).
 *
 * The reference (nh13/DWGSIM) has no plugin/FFI layer; its seam is the single call
 * dwgsim_core(dwgsim_opt_t*) (src/dwgsim.c:419, called at :1163) and inside it
 * mut_diref() (src/mut.c:591, called at dwgsim.c:629) followed by the inlined per-pair loop
 * (dwgsim.c:636-1099).  The entry points below are what a host-side binding for that seam
 * binds: plain pointers and sizes, no C++/torch types, error codes
 * instead of exit(1) (the reference's messages are available through dwgsim_hip_last_error).
 *
 * Random numbers: Philox4x32-10 keyed by (seed, contig) and counter
 * (index, retry, domain|attempt, block) -- see DESIGN.md "RNG layout".  Any read-index range
 * of any contig can be generated independently and in any order.
 *
 * Threading: a context is single-owner; different contexts (one per GPU) may be used
 * concurrently.  There is no global state.
 */
#ifndef DWGSIM_HIP_H
#define DWGSIM_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWGSIM_HIP_ABI_VERSION 11

/* error codes (negative) */
#define DWGSIM_HIP_OK            0
#define DWGSIM_HIP_ERR_ARG      -1   /* bad argument / option out of range (dwgsim_opt.c:307-371) */
#define DWGSIM_HIP_ERR_DEVICE   -2   /* no usable HIP device / HIP runtime error */
#define DWGSIM_HIP_ERR_NOMEM    -3
#define DWGSIM_HIP_ERR_UNSUP    -4   /* option outside the accelerated path (see DESIGN.md "out of scope") */
#define DWGSIM_HIP_ERR_FAILED   -5   /* "failed to generate a read after %d trials" (dwgsim.c:837-840) */
#define DWGSIM_HIP_SLOTS 4          /* output sets of a context: batches that can be in flight (kernels | copy-out issued, twice | copy-out landing) */
#define DWGSIM_HIP_ERR_STATE    -6   /* call order violated (e.g. simulate before mutate) */

/* Why dwgsim_core() passes over a contig (dwgsim.c:539-625, the "[dwgsim_core] #k skip sequence" notes): returned in place of a pair count by
 * dwgsim_hip_pairs_for_contig, dwgsim_hip_contig_region_length and dwgsim_hip_job_add_contig.  A range of their own, disjoint from the error
 * codes above: a skipped contig is not a failure, and a failure must never be mistaken for a skipped contig. */
#define DWGSIM_HIP_SKIP_NO_REGION    -100  /* #0: the contig is not in the targeted region (-x) */
#define DWGSIM_HIP_SKIP_NON_ACGT     -101  /* #1: more than 95 % of its targeted bases are non-ACGT */
#define DWGSIM_HIP_SKIP_AMPLICON     -102  /* #2: shorter than the read length (-a) */
#define DWGSIM_HIP_SKIP_SHORT_INSERT -103  /* #3: shorter than dist + 3 std_dev */
#define DWGSIM_HIP_SKIP_SHORT_READ   -104  /* #4: shorter than a read */
#define DWGSIM_HIP_SKIP_NO_PAIRS     -105  /* #5: a negative pair count */
#define DWGSIM_HIP_IS_SKIP(r) ((r) <= -100 && (r) >= -105)

/* POD mirror of the dwgsim_opt_t fields read on the path (src/dwgsim_opt.h:21-60);
 * defaults are those of dwgsim_opt_init() (src/dwgsim_opt.c:40-80). */
typedef struct dwgsim_hip_params {
    double  e_start[2], e_end[2];   /* -e / -E  per-base error rate ramp (start..end) of read 1 / 2   */
    int32_t is_inner;               /* -i */
    int32_t dist;                   /* -d */
    double  std_dev;                /* -s */
    int64_t N;                      /* -N (-1: use C) */
    double  C;                      /* -C (-1: use N) */
    int32_t length[2];              /* -1 / -2 */
    double  mut_rate;               /* -r */
    double  mut_freq;               /* -F */
    double  indel_frac;             /* -R */
    double  indel_extend;           /* -X */
    int32_t indel_min;              /* -I */
    double  rand_read;              /* -y */
    int32_t max_n;                  /* -n */
    int32_t data_type;              /* -c 0 Illumina, 1 SOLiD, 2 Ion Torrent */
    int32_t strandedness;           /* -S */
    int32_t read_one_strand;        /* -A */
    int32_t is_hap;                 /* -H */
    int32_t seed;                   /* -z (must be >= 0 here: the CLI resolves -1 to time(0)) */
    int32_t fixed_quality;          /* -q as a character code, or -1 */
    double  quality_std;            /* -Q */
    int32_t reads_output_type;      /* -o 0 all, 1 bwa only, 2 bfast only */
    int32_t output_type;            /* -M 0 all, 1 reads only, 2 mutations only */
    int32_t amplicons;              /* -a */
    const char *read_prefix;        /* -P or NULL */
    const char *flow_order;         /* -f or NULL */
    int32_t use_base_error;         /* -B */
} dwgsim_hip_params_t;

typedef struct dwgsim_hip_ctx dwgsim_hip_ctx_t;

/* output streams of one simulate() batch */
enum { DWGSIM_HIP_STREAM_BWA1 = 0, DWGSIM_HIP_STREAM_BWA2 = 1, DWGSIM_HIP_STREAM_BFAST = 2,
       DWGSIM_HIP_STREAM_SAM = 3 /* (ABI 8) the truth SAM: only with dwgsim_hip_set_truth_sam(ctx, 1) */ };

typedef struct dwgsim_hip_batch {
    uint64_t n_pairs;          /* pairs generated (== requested) */
    uint64_t n_random;         /* how many of them are random reads ("rand_ii" increment, dwgsim.c:1096) */
    uint64_t n_retries;        /* rejected attempts (N filter / walk off the contig, dwgsim.c:833-842) */
    uint64_t bytes[3];         /* finished FASTQ text bytes per stream (0 if the stream is disabled) */
    const void *dev_ptr[3];    /* device addresses of the packed text (valid until the slot is reused) */
    float    kernel_ms;        /* HIP-event time of the batch's kernels on the context's stream (simulate_pairs, the abort-rule epilogue, the gzip kernels) */
    float    sim_kernel_ms;    /* ... of the dominant kernel (simulate_pairs) alone */
    /* The reference's abort rule (one counter of failed attempts over the pairs of a contig, reset by every genomic read, fatal above
     * 10 000: dwgsim.c:635, :833-843) as a mergeable summary of THIS batch alone: {fails before its first reset (all of them if it has
     * none), fails after its last reset, has a reset, a run between two of its resets passed the limit}.  A host that shards one contig
     * over several contexts joins the summaries in read-index order (dwgsim_hip_failseg_join) to get the exact verdict. */
    uint64_t fail_seg[4];
    uint64_t fail_carry;       /* the counter after this batch, given the carry it started from */
    uint64_t gz_bytes[3];      /* with dwgsim_hip_set_gzip(ctx, 1): bytes of the .gz form of each stream (a sequence of complete gzip members) */
    /* (ABI 8) with dwgsim_hip_set_truth_sam(ctx, 1): stream DWGSIM_HIP_STREAM_SAM -- its text bytes, the bytes of its .gz form, its device address (else 0, 0, NULL) */
    uint64_t sam_bytes, sam_gz_bytes;
    const void *sam_dev_ptr;
} dwgsim_hip_batch_t;

/* rand_base value meaning "continue the running count after the previous batch of this context" (kept on the device, so successive
 * batches can be enqueued without a host round trip) */
#define DWGSIM_HIP_RAND_CHAIN UINT64_MAX

/* dwgsim_opt_init() defaults (dwgsim_opt.c:40-80) */
void dwgsim_hip_params_default(dwgsim_hip_params_t *p);

/* Range/consistency checks of dwgsim_opt_parse() (dwgsim_opt.c:307-371, :396-413, :463-469).
 * Returns DWGSIM_HIP_OK or DWGSIM_HIP_ERR_ARG / _UNSUP; msg (optional, cap bytes) receives the
 * reference's message text. */
int dwgsim_hip_params_check(const dwgsim_hip_params_t *p, char *msg, size_t cap);

/* Pairs to simulate on a contig of length l: dwgsim.c:535-537, :582-590 and the skip rules
 * #2-#5 (:595-623).  Returns n_pairs (>= 0), or DWGSIM_HIP_SKIP_AMPLICON / _SHORT_INSERT / _SHORT_READ / _NO_PAIRS for skip rule #2 .. #5
 * (skipped contigs get no mutations either, dwgsim.c:605-611). */
int64_t dwgsim_hip_pairs_for_contig(const dwgsim_hip_params_t *p, int64_t l, uint64_t tot_len,
                                    int is_last_contig, int64_t n_sim_so_far);

/* Replaces the allocation/teardown half of dwgsim_core (dwgsim.c:442-453, :1103-1120).
 * device = HIP device ordinal.  Fails (NULL, *err set) when no GPU is present. */
dwgsim_hip_ctx_t *dwgsim_hip_create(const dwgsim_hip_params_t *p, int device, int *err);
void dwgsim_hip_destroy(dwgsim_hip_ctx_t *ctx);
/* The parameters the context works with: those it was created from, with the error rates -B calibrated (dwgsim_opt.c:452-454: e.start = e.end =
 * the scaled rate).  read_prefix / flow_order come back NULL (the context keeps its own copies). */
int dwgsim_hip_get_params(const dwgsim_hip_ctx_t *ctx, dwgsim_hip_params_t *out);
const char *dwgsim_hip_last_error(const dwgsim_hip_ctx_t *ctx);

/* Replaces seq_read_fasta()'s result + nst_nt4_table lookup (mut.c:49-87, dwgsim.c:56-73):
 * ascii[0..len) are the contig's sequence characters (caller keeps ownership); the packed bases
 * stay resident in HBM.  contig_index = 0-based ordinal of the contig in the FASTA (RNG key).
 * Returns a handle >= 0 or an error code. */
int dwgsim_hip_add_contig(dwgsim_hip_ctx_t *ctx, const char *name, const uint8_t *ascii, int64_t len,
                          uint32_t contig_index);
/* Releases the contig's group.  Every batch that reads the group must have been waited for (dwgsim_hip_wait): DWGSIM_HIP_ERR_STATE otherwise. */
int dwgsim_hip_drop_contig(dwgsim_hip_ctx_t *ctx, int contig);

/* Several contigs at once -- a GROUP.  The reference's contig loop (dwgsim.c:519-625) costs nothing per contig beyond a calloc; here a contig
 * that is added alone costs a chain of walk kernels, a launch and a host synchronisation of its own, which a scaffold-level assembly (10^3-10^5
 * contigs) cannot afford.  The contigs of one call are resident together: dwgsim_hip_mutate_contig on any of them walks all of them with ONE
 * chain of kernels, and read-index ranges of several of them can be simulated by ONE launch (dwgsim_hip_simulate_ranges_async).  Returns the
 * handle of the first contig; contig k of the call has handle + k.  dwgsim_hip_drop_contig on any of them releases the whole group.
 * Upload: if the n buffers already are the group layout inside one page-locked allocation (dwgsim_hip_host_alloc; ascii[k] == ascii[0] +
 * starts[k] of dwgsim_hip_group_layout, zero bytes between the contigs) the copy is asynchronous and the buffers must stay unchanged until
 * dwgsim_hip_mutate_wait returned for the group; any other buffers may be released when the call returns. */
int dwgsim_hip_add_contigs(dwgsim_hip_ctx_t *ctx, int n, const char *const *names, const uint8_t *const *ascii, const int64_t *lens,
                           const uint32_t *contig_index);
/* Where the contigs of a group lie in its coordinate space: starts[k] (optional) = first byte of contig k; returns the total size. */
int64_t dwgsim_hip_group_layout(const int64_t *lens, int n, int64_t *starts);

/* Replaces regions_bed_init() (src/regions_bed.c:38-125, dwgsim.c:499-506): target regions (-x).  names/lens as for
 * dwgsim_hip_set_mutation_input.  *total_len receives the summed region length (the reference's tot_len, dwgsim.c:502-505).
 * Call before add_contig. */
int dwgsim_hip_set_regions(dwgsim_hip_ctx_t *ctx, const char *path, const char *const *names, const int64_t *lens,
                           int n_contigs, uint64_t *total_len);

/* dwgsim.c:539-581: the region length of a contig -- the `l` the reference then uses for pairs-per-contig, the skip rules
 * and fragment placement -- or DWGSIM_HIP_SKIP_NO_REGION (skip #0) / DWGSIM_HIP_SKIP_NON_ACGT (skip #1: > 95 % non-ACGT).  non_acgt / region_bases
 * (optional) receive the two numbers the reference prints with skip #1 (num_n and the region length, dwgsim.c:574-576). */
int64_t dwgsim_hip_contig_region_length(dwgsim_hip_ctx_t *ctx, uint32_t contig_index, const uint8_t *ascii, int64_t len, int64_t *non_acgt, int64_t *region_bases);

/* The `l` that sizes fragment placement on this contig (dwgsim.c:659-671): defaults to the contig length, or to its region
 * length once regions are set.  The reference's last contig in -N mode keeps the full length (dwgsim.c:535-537 bypasses the
 * region bookkeeping): a caller mirroring that passes len here. */
int dwgsim_hip_contig_set_placement_length(dwgsim_hip_ctx_t *ctx, int contig, int64_t l);

/* Replaces muts_input_init() (src/mut_input.c:47-67, called at dwgsim.c:494-497): read a mutation file that then drives
 * mutate_contig instead of the random walk (mut.c:644-745).  type: 0 = bed (-b), 1 = txt (-m), 2 = vcf (-v).
 * names/lens = every contig of the FASTA in file order (the reference's contigs_add table, dwgsim.c:474-476). */
int dwgsim_hip_set_mutation_input(dwgsim_hip_ctx_t *ctx, int type, const char *path, const char *const *names,
                                  const int64_t *lens, int n_contigs);

/* Replaces mut_diref() random branch + mut_left_justify() (mut.c:591-643, :481-589): builds the
 * two mutated haplotypes of the contig in HBM. */
int dwgsim_hip_mutate_contig(dwgsim_hip_ctx_t *ctx, int contig);
/* The same in two halves (the walk runs on a stream of its own: a group can be uploaded and walked while batches of another group are being
 * simulated): mutate_async enqueues, mutate_wait blocks until the haplotypes are finished and reports the walk's errors.  `contig` = any
 * contig of the group; the whole group is walked. */
int dwgsim_hip_mutate_async(dwgsim_hip_ctx_t *ctx, int contig);
int dwgsim_hip_mutate_wait(dwgsim_hip_ctx_t *ctx, int contig);
/* 1: the enqueued walk has finished on the device (mutate_wait will not block; a capacity re-run, rare, may still follow inside it), 0: not yet */
int dwgsim_hip_mutate_poll(dwgsim_hip_ctx_t *ctx, int contig);

/* Replaces mut_print() (mut.c:781-893): the mutations.txt and mutations.vcf BODY lines of this
 * contig.  Buffers are owned by the context and valid until the next call for any contig. */
int dwgsim_hip_mutations_text(dwgsim_hip_ctx_t *ctx, int contig, const char **txt, size_t *txt_len,
                              const char **vcf, size_t *vcf_len);
/* mut_print() in two halves, for a caller that keeps the device busy meanwhile (the job level does): `take` fetches the list of mutated cells of
 * the contig's whole GROUP (device work, on the calling thread) and returns it as an object of its own (NULL: see last_error; *n_contigs =
 * contigs of the group, in the order they were added); `mutlist_text` makes the mutations.txt / .vcf body lines of the group's k-th contig
 * from it -- it touches neither the context nor the device, so any thread may call it while the context simulates the group's reads.  The
 * buffers belong to the list and are valid until the next call on the same list. */
typedef struct dwgsim_hip_mutlist dwgsim_hip_mutlist_t;
dwgsim_hip_mutlist_t *dwgsim_hip_mutations_take(dwgsim_hip_ctx_t *ctx, int contig, int *n_contigs);
int dwgsim_hip_mutlist_text(dwgsim_hip_mutlist_t *list, int k, const char **txt, size_t *txt_len, const char **vcf, size_t *vcf_len);
void dwgsim_hip_mutlist_free(dwgsim_hip_mutlist_t *list);

/* (ABI 6) The two mutated haplotypes as FASTA text, assembled on the device from the finished cells (no counterpart in the reference; DESIGN.md "6d").
 * The reads are drawn from the cells, so the text restates them, forward strand: an unmutated or substituted cell gives its base, a deleted cell
 * nothing, a cell with an insertion its own base and then the inserted bases in the order mutations.txt prints them.  The cells hold base codes:
 * A, C, G and T come back as upper case, every other character of the input (lower-case letters are folded first; N, IUPAC codes, '-', '.') as N.
 * One record per contig of the group, in the order they were added: '>' + the contig's name + '\n' (the plain name: no -P prefix), then the bases in
 * lines of `width` characters, each line ended by '\n' (width 0: the whole sequence on one line; a haplotype without bases has the header line alone).
 * haplotype_fasta builds the text of haplotype `hap` (0 or 1) of the whole GROUP `contig` belongs to; it stays in device memory, *bytes (optional) = its
 * size.  DWGSIM_HIP_ERR_STATE before the group's walk has finished, DWGSIM_HIP_ERR_ARG for another hap or a negative width.  The text is kept per group
 * and haplotype until the group is dropped or walked again: a call with the same width finds it there, one with another width builds it again.
 * haplotype_layout (after haplotype_fasta for that group and hap): where the contig's record lies in the group's text (offset, bytes; header included)
 * and the haplotype's length in bases; any of the three may be NULL.
 * haplotype_fetch copies n bytes from `offset` of the text the LAST haplotype_fasta call for `hap` built or found, to host memory: a page-locked
 * destination directly, a pageable one through the context's page-locked staging (as dwgsim_hip_fetch).  DWGSIM_HIP_ERR_ARG past the end of the text. */
int dwgsim_hip_haplotype_fasta(dwgsim_hip_ctx_t *ctx, int contig, int hap, int width, uint64_t *bytes);
int dwgsim_hip_haplotype_layout(dwgsim_hip_ctx_t *ctx, int contig, int hap, uint64_t *offset, uint64_t *bytes, int64_t *bases);
int dwgsim_hip_haplotype_fetch(dwgsim_hip_ctx_t *ctx, int hap, uint64_t offset, void *host_dst, size_t n);

/* (ABI 11) The map between a haplotype (dwgsim_hip_haplotype_fasta) and the reference, as a UCSC chain (no counterpart in the reference; DESIGN.md "6g").
 * A cell of the haplotype is ALIGNED unless it is deleted: its own base stands opposite the reference base of the cell; the n > 0 bases inserted behind a
 * cell stand opposite nothing.  An ungapped BLOCK is a maximal run of consecutive aligned cells s .. e in which no cell but e has inserted bases behind it.
 * Block k of a contig of l cells is {size = e - s + 1, d_ref, d_hap}: d_ref the deleted cells and d_hap the inserted bases between it and block k + 1 -- for
 * the LAST block what lies behind it, the deleted cells up to the contig's end and the bases inserted behind e, which are not part of the chain.  So
 * ref_start + the sum of size + d_ref is l, and the sum of size + d_hap is the haplotype's length.
 * haplotype_chain finds the blocks of haplotype `hap` (0 or 1) of the whole GROUP `contig` belongs to (two passes over its cells on the device; the block ends
 * come to the host, which pairs them); *blocks (optional) = their number in the group.  They are kept per group and haplotype until the group is dropped or
 * walked again: a second call finds them there.  DWGSIM_HIP_ERR_STATE before the group's walk has finished, DWGSIM_HIP_ERR_ARG for another hap.
 * chain_blocks (after haplotype_chain for that group and hap: DWGSIM_HIP_ERR_STATE else): the blocks of one contig.  *n = their number (0: every cell of the
 * haplotype is deleted -- it has no chain), *ref_start = the first aligned cell; the first min(*n, cap) blocks are copied to `blocks` (NULL with cap 0: ask
 * for the number).  Any of n, ref_start may be NULL. */
typedef struct dwgsim_hip_chain_block { int64_t size, d_ref, d_hap; } dwgsim_hip_chain_block_t;
int dwgsim_hip_haplotype_chain(dwgsim_hip_ctx_t *ctx, int contig, int hap, uint64_t *blocks);
int dwgsim_hip_chain_blocks(dwgsim_hip_ctx_t *ctx, int contig, int hap, uint64_t *n, int64_t *ref_start, dwgsim_hip_chain_block_t *blocks, uint64_t cap);
/* The chain of one contig as text, from the blocks above (n > 0).  direction DWGSIM_HIP_CHAIN_FROM_REF: target the reference, query the haplotype --
 *     chain <score> <name> <l> + <ref_start> <ref_end> <name> <hap_len> + 0 <hap_end> <id>\n
 *     <size>\t<d_ref>\t<d_hap>\n      a line per block but the last
 *     <size>\n\n                       the last block, and the empty line that ends a chain
 * score = the sum of the sizes; hap_end = hap_len - the last block's d_hap; ref_end = l - the last block's d_ref.  DWGSIM_HIP_CHAIN_TO_REF (what liftOver wants
 * for coordinates on the haplotype FASTA): the same chain with target and query exchanged -- the two groups of name, size, strand, start, end swapped and every
 * block line <size>\t<d_hap>\t<d_ref>.  Needs no context.  Returns the size of the text (no terminating 0) and writes it when buf has room for it (cap >= the
 * size); a negative DWGSIM_HIP_ERR_ARG for n = 0, a NULL name or blocks, another direction, or blocks that do not add up to l. */
#define DWGSIM_HIP_CHAIN_TO_REF 0
#define DWGSIM_HIP_CHAIN_FROM_REF 1
int64_t dwgsim_hip_chain_format(const char *name, int64_t l, int64_t ref_start, const dwgsim_hip_chain_block_t *blocks, uint64_t n, int direction, uint64_t id,
                                char *buf, size_t cap);

/* Number of random reads among pairs [first_ii, first_ii + n_pairs) of the contig (for sharding:
 * rand_ii is a running count over all earlier pairs, dwgsim.c:1042,1096). */
int dwgsim_hip_count_random(dwgsim_hip_ctx_t *ctx, int contig, uint64_t first_ii, uint64_t n_pairs,
                            uint64_t *n_random);

/* A read-index range of one contig.  A call that takes several of them covers them in the order given (= file order); they must belong to
 * contigs of one group. */
typedef struct dwgsim_hip_range { int32_t contig; int32_t reserved; uint64_t first_ii, n_pairs; } dwgsim_hip_range_t;
/* random reads among the pairs of the ranges: their total, and (per_range != NULL) one count per range */
int dwgsim_hip_count_random_ranges(dwgsim_hip_ctx_t *ctx, const dwgsim_hip_range_t *ranges, int n_ranges, uint64_t *n_random, uint64_t *per_range);

/* Replaces the loop body dwgsim.c:636-1099 for the read-index range [first_ii, first_ii+n_pairs)
 * of one contig.  rand_base = number of random reads emitted before first_ii (over all contigs).
 * slot in 0 .. DWGSIM_HIP_SLOTS - 1: which of the context's output sets to fill.  Blocking form:
 * returns after the kernels completed; FASTQ text stays in HBM (out->dev_ptr) until a fetch copies it out.
 * Replaces, together with the fetch calls, the gzprintf / gzputc stream of dwgsim.c:919-981. */
int dwgsim_hip_simulate(dwgsim_hip_ctx_t *ctx, int contig, uint64_t first_ii, uint64_t n_pairs,
                        uint64_t rand_base, int slot, dwgsim_hip_batch_t *out);

/* The same in two halves, so that several batches can be in flight (one per slot): simulate_async only enqueues -- kernels, the abort-rule
 * epilogue and the read-back of the batch's counters on the context's compute stream -- and returns; wait blocks until that batch has
 * finished, reports its errors and fills *out.  Batch k+1 may be enqueued (other slot, rand_base = DWGSIM_HIP_RAND_CHAIN) before
 * batch k was waited for; a slot is reused only after its wait(), and its kernels wait on the device for any fetch still reading it. */
int dwgsim_hip_simulate_async(dwgsim_hip_ctx_t *ctx, int contig, uint64_t first_ii, uint64_t n_pairs,
                              uint64_t rand_base, int slot);
int dwgsim_hip_wait(dwgsim_hip_ctx_t *ctx, int slot, dwgsim_hip_batch_t *out);
/* ... for several ranges at once: one launch, one contiguous piece of every output stream (the loop dwgsim.c:519-1099 over several
 * contigs).  The abort rule's counter starts from zero wherever a range begins its contig (first_ii == 0), as `int num_failed = 0` does at
 * dwgsim.c:635; rand_base counts the random reads in front of the first range.
 * ONE call takes at most 2^31 blocks of pairs; Illumina / SOLiD: and only as many pairs as leave the sum of their random reads and the bytes of their first output
 * stream in 62 bits together (the kernels' one look-back word: at 2 x 150 bp 2^26 pairs, 50 GB of text per stream) -- beyond either: DWGSIM_HIP_ERR_ARG
 * "too many pairs in one call"; a job is cut into calls long before (dwgsim_hip_job_*: 2^18 pairs each). */
int dwgsim_hip_simulate_ranges_async(dwgsim_hip_ctx_t *ctx, const dwgsim_hip_range_t *ranges, int n_ranges, uint64_t rand_base, int slot);

/* The failure counter carried into the next simulate call (default: the previous batch's counter when the call continues the
 * same contig at the next read index, else 0).  For sharded jobs: the carry out of the preceding shard. */
int dwgsim_hip_set_fail_carry(dwgsim_hip_ctx_t *ctx, uint64_t carry);

/* acc = acc . next in read-index order (both as dwgsim_hip_batch_t::fail_seg).  Returns 1 when the joined run passes the limit
 * (the reference would have aborted), else 0.  Start from {carry, carry, 0, 0}. */
int dwgsim_hip_failseg_join(uint64_t acc[4], const uint64_t next[4]);

/* Contiguous near-equal read-index ranges, in order: shard `rank` of `world` over [0, n_pairs). */
void dwgsim_hip_shard_range(uint64_t n_pairs, int rank, int world, uint64_t *first, uint64_t *n);

/* Page-locked host memory for fetch destinations (hipHostMalloc / hipHostFree for callers that do not link the HIP runtime). */
void *dwgsim_hip_host_alloc(size_t bytes);
void dwgsim_hip_host_free(void *p);

/* Asynchronous copy of one finished stream of a waited-for slot into PAGE-LOCKED host memory, on the context's copy stream (it
 * overlaps with the kernels of the other slot); fetch_wait blocks until every copy enqueued for the slot has landed. */
int dwgsim_hip_fetch_async(dwgsim_hip_ctx_t *ctx, int slot, int stream, void *host_dst, size_t cap);
int dwgsim_hip_fetch_wait(dwgsim_hip_ctx_t *ctx, int slot);

/* gzip on the GPU (replaces the gzopen / gzprintf / gzputc output of dwgsim.c:919-981, :1150-1158): once switched on, every simulate call also
 * leaves each finished stream in HBM as a sequence of complete gzip members (one per 32 KiB of text, dynamic Huffman codes; concatenating the
 * members of successive batches gives a valid .gz whose decompressed bytes are exactly the text), and fetch_gz_async copies THAT to page-locked
 * host memory: half of the bytes cross PCIe and the host only writes them. */
int dwgsim_hip_set_gzip(dwgsim_hip_ctx_t *ctx, int on);
int dwgsim_hip_fetch_gz_async(dwgsim_hip_ctx_t *ctx, int slot, int stream, void *host_dst, size_t cap);

/* (ABI 8) The truth SAM: the true alignment of every simulated read end, made on the device behind the batch's kernels (no counterpart in the reference;
 * DESIGN.md "6e").  Once switched on, every simulate call also leaves stream DWGSIM_HIP_STREAM_SAM in HBM: one SAM record per read end, in pair order (end 1,
 * then end 2), without a header.  fetch, fetch_async, fetch_gz_async (with dwgsim_hip_set_gzip: members like the other streams') and debug_count_byte take
 * the stream; while the feature is off they answer DWGSIM_HIP_ERR_ARG for it.  Illumina reads only: DWGSIM_HIP_ERR_UNSUP for -c 1 / -c 2.
 * DWGSIM_HIP_ERR_STATE while a batch is in flight.  Off (the default): nothing is launched or allocated, every byte is as before.
 * A record: QNAME = the FASTQ name without '@' and "/1" / "/2"; FLAG = 0x1 | 0x2 | 0x40 / 0x80 | 0x10 (the end's strand) | 0x20 (the mate's), single-end
 * 0 / 0x10; RNAME = the contig's plain name; POS = the leftmost reference cell that gives an M, 1-based; MAPQ 60; CIGAR: M an unmutated or substituted cell,
 * D a deleted cell, I inserted bases, equal neighbours merged -- it never starts or ends with D and always holds an M, and it starts or ends with I where
 * the read stops inside an insertion; RNEXT "=", PNEXT the mate's POS, TLEN rightmost end - leftmost start + 1, positive for the leftmost end (end 1 on
 * a tie); SEQ / QUAL the FASTQ's, reverse-complemented / reversed under 0x10; HP:i:1 or HP:i:2, the haplotype the read was drawn from.  A random read:
 * FLAG 0x4 (pairs: 0x1 | 0x4 | 0x8 | 0x40 / 0x80), RNAME *, POS 0, MAPQ 0, CIGAR *, RNEXT *, PNEXT 0, TLEN 0, no HP. */
int dwgsim_hip_set_truth_sam(dwgsim_hip_ctx_t *ctx, int on);
/* (ABI 9) NM and MD on top of the truth SAM: with it, every mapped record carries NM:i:<n> and MD:Z:<string> behind HP:i:, in that order; unmapped (random-read)
 * records get no tags.  It takes effect only while the truth SAM is on and on its own produces no stream; off (the default), every byte of every output is as
 * before and no kernel launch is added.  DWGSIM_HIP_ERR_STATE while a batch is in flight, DWGSIM_HIP_ERR_UNSUP for -c 1 / -c 2.
 * The law (samtools calmd's convention, restated).  Walk the record's CIGAR in reference order from POS.  r = the reference letter of a cell: A C G T for the
 * codes 0-3, N for everything else, always upper case.  b = the base of SEQ as the line prints it (reverse-complemented under 0x10); a leading I run takes the
 * first bases of SEQ.  An M cell matches if and only if b == r and r is one of ACGT (N against N is a mismatch): a match adds one to the running count; a
 * mismatch emits the count, then r, sets the count to 0 and adds 1 to NM.  An I run of n bases: NM += n, MD untouched, the count runs on.  A D run of n cells:
 * the count, '^', the n reference letters; the count is 0 again; NM += n.  At the end the count, also when it is 0.  So MD matches
 * [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)* and a mismatch directly behind a deletion gets its 0 (^AC0T).  SEQ holds the sequencing errors, so the tags show them too.
 * MD spells out every deleted base, so a line has no bound in the read length: a batch whose text outgrows its planned buffer is run a second time inside
 * dwgsim_hip_wait with the exact room (nothing is lost, nothing of the job's random numbers moves); a batch whose SAM would pass 4 GiB is refused with
 * DWGSIM_HIP_ERR_UNSUP (use smaller batches). */
int dwgsim_hip_set_truth_md(dwgsim_hip_ctx_t *ctx, int on);
/* The header that goes in front of the records: @HD VN:1.6 SO:unsorted GO:query, one @SQ per contig of the table (every contig of the FASTA, in its
 * order, skipped ones included), one @PG.  Needs no context.  Returns the header's size; at most cap bytes of it are written to buf (NULL with cap 0: the
 * size alone). */
int64_t dwgsim_hip_truth_sam_header(const char *const *names, const int64_t *lens, int n, char *buf, size_t cap);
/* (ABI 10) The true read depth of every simulated variant, the counters behind <prefix>.truth.vcf (DESIGN.md "6f").  Switched on, every simulate call adds to
 * two 64-bit counters per listed mutated cell of its group, on the device, from the replayed alignments of the reads it made -- with or without the truth SAM,
 * whose every output byte stays as it is.  The rule (stated once, next to the kernel: dw_truth.hpp k_truth_depth): a mapped read end of haplotype h aligned to
 * the cells lo .. hi adds 1 to counter h of every listed cell in lo .. hi; where haplotype h has an insertion at hi the end counts there only if it holds all
 * inserted bases.  Deleted cells inside lo .. hi count (the read spans the deletion); random reads count nowhere; sequencing errors are not looked at (depth by
 * origin, not by observed base).  A batch counts once, also when dwgsim_hip_wait runs it a second time.  Illumina reads only: DWGSIM_HIP_ERR_UNSUP for -c 1 /
 * -c 2; DWGSIM_HIP_ERR_STATE while a batch is in flight.  Off (the default): nothing is launched or allocated, every byte is as before. */
int dwgsim_hip_set_truth_depth(dwgsim_hip_ctx_t *ctx, int on);
/* ... the counters of one contig: its slice of the group's list of mutated cells (the cells dwgsim_hip_mutations_text walks, reference codes outside ACGT
 * included), in list order, two per cell: haplotype 1, haplotype 2.  They hold everything this context has simulated for the contig since its walk; the call
 * waits for the batches the context has enqueued.  Returns the cells of the slice; at most cap_cells of them (2 cap_cells words) are written to counts (NULL
 * with cap_cells 0: the size alone).  DWGSIM_HIP_ERR_ARG while the feature is off. */
int64_t dwgsim_hip_truth_depth_fetch(dwgsim_hip_ctx_t *ctx, int contig, uint64_t *counts, size_t cap_cells);
/* ... the records of the truth VCF for contig k of a list taken with dwgsim_hip_mutations_take: the lines dwgsim_hip_mutlist_text gives as vcf, each with
 * "GT:AD:DP" and one sample column behind it.  counts: the contig's n_cells cells as dwgsim_hip_truth_depth_fetch gave them -- or the sum of what several
 * contexts gave (DWGSIM_HIP_ERR_ARG when n_cells is not the contig's slice); NULL: every counter 0.  GT 1|0, 0|1, 1|1 for pl = 1, 2, 3; AD ref,alt: alt the ends of the haplotype(s)
 * that carry the record's allele, ref those of the other haplotype where its cell is unmutated, else 0; DP both counters.  A deletion's record takes the
 * counters of the first deleted cell of its run.  No context, no device.  The text is valid until the next call for the list. */
int dwgsim_hip_mutlist_truth_vcf_text(dwgsim_hip_mutlist_t *list, int k, const uint64_t *counts, size_t n_cells, const char **vcf, size_t *vcf_len);
/* ... and the header in front of them: that of mutations.vcf with three ##FORMAT lines (GT, AD, DP) in front of #CHROM and "FORMAT" and the sample name
 * "dwgsim" behind INFO.  Called like dwgsim_hip_truth_sam_header. */
int64_t dwgsim_hip_truth_vcf_header(const char *const *names, const int64_t *lens, int n, char *buf, size_t cap);

/* Copy one finished stream of a slot to host memory.  A page-locked destination (hipHostMalloc / hipHostRegister) takes one direct
 * hipMemcpyAsync at link speed; pageable memory goes through double-buffered pinned staging inside. */
int dwgsim_hip_fetch(dwgsim_hip_ctx_t *ctx, int slot, int stream, void *host_dst, size_t cap);

/* Library / device info for logs: returns the ABI version; name gets the HIP device name. */
/* The NUMA node of the host the device hangs off (/sys/bus/pci/devices/<bus id>/numa_node), -1 when unknown.  The job level runs each device's worker
 * thread -- which allocates and fills that device's page-locked buffers -- on the cores of this node.  (No counterpart in the reference: it has one thread.) */
int dwgsim_hip_device_numa_node(int device);
int dwgsim_hip_device_info(int device, char *name, size_t cap, int *n_cu, size_t *hbm_bytes);
/* HIP devices visible to the process (0 without a GPU). */
int dwgsim_hip_device_count(void);

/* ------------------------------------------------------------------------------------------------------------------------------------
 * Job level: dwgsim_core() (dwgsim.c:419-1121) as a whole, on any number of GPUs.  The calls above drive ONE device and leave the
 * choreography to the caller; these own it: contig scheduling (dwgsim.c:519-625), grouping of small contigs, upload / walk / simulate /
 * copy-out pipelines of every device, read-index sharding (batch b of a group's pairs belongs to device b mod n; every device walks the
 * group itself; the random-read count in front of a batch and the abort rule's summaries are the only things that cross devices, as host
 * integers -- no collective), and delivery of the output in file order.  A binding at the reference's seam (dwgsim.c:1163) is: create, set the
 * contig table, add every contig of the FASTA in order, finish.
 * ------------------------------------------------------------------------------------------------------------------------------------ */
typedef struct dwgsim_hip_job dwgsim_hip_job_t;

typedef struct dwgsim_hip_job_sink {
    void *user;
    /* mut_print() (mut.c:781-893): the mutations.txt / mutations.vcf body lines of the next contig, contigs in FASTA order.  One call at a
     * time, from a thread of the job.  Non-zero return stops the job. */
    int (*mutations)(void *user, const char *contig, const char *txt, size_t txt_len, const char *vcf, size_t vcf_len);
    /* The gzprintf / gzputc stream of dwgsim.c:919-981: the next piece of output stream `stream` (DWGSIM_HIP_STREAM_*), pieces in file
     * order.  gz != 0: `len` bytes of complete gzip members that hold text_len bytes of text; gz == 0: len == text_len bytes of text.
     * One thread per stream, so the three files can be written side by side; `data` is page-locked memory of the job, reused once the call
     * has returned.  NULL: the reads are simulated and left on the device (benchmarks).  Non-zero return stops the job. */
    int (*reads)(void *user, int stream, const void *data, size_t len, size_t text_len, int gz);
    /* dwgsim_core's stderr lines (skip notes, the running pair count); NULL: written to stderr unless options.quiet */
    void (*message)(void *user, const char *text);
    /* (ABI 5) Instead of reads, for a sink that can take pieces OUT OF ORDER (pwrite): `offset` = where this piece goes in output stream `stream` as it is
     * delivered (the members back to back, or the text).  Called CONCURRENTLY, by one thread per device and stream -- every device hands over what it made
     * itself -- each piece exactly once, in any order; together the pieces tile [0, total) of each stream.  The ordered form has one thread per stream, and
     * a sink that touches the bytes takes 21-26 GB/s from it (measured, memcpy: profiles/r06_solo_rank_entry.txt): less than one device's link delivers, so at
     * N > 1 devices it would be the job's ceiling.  Used when reads_at != NULL (reads is then ignored).  Non-zero return stops the job. */
    int (*reads_at)(void *user, int stream, uint64_t offset, const void *data, size_t len, size_t text_len, int gz);
} dwgsim_hip_job_sink_t;

typedef struct dwgsim_hip_job_options {
    int32_t  gzip;           /* 1: reads() gets gzip members made on the GPU (dwgsim_hip_set_gzip), 0: text */
    int32_t  quiet;
    uint64_t batch_pairs;    /* pairs per launch (0: 2^18) */
    uint64_t group_bp;       /* consecutive contigs are resident, walked and simulated together up to this many bases (0: 32 Mi) */
    uint64_t min_share;      /* a group is spread over fewer devices while a device's share would stay below this many pairs (0: 65536) */
} dwgsim_hip_job_options_t;

/* (ABI 6) The mutated haplotypes as FASTA (dwgsim_hip_haplotype_fasta), through a call of its own: dwgsim_hip_job_sink_t has no size member, so it
 * cannot grow.  fn gets the next piece of the file of haplotype `hap` (0 or 1): the pieces of one haplotype arrive in file order, each at most 32 MiB,
 * from ONE thread of the job (pieces of the two haplotypes alternate group by group); `data` is page-locked memory of the job, reused once the call
 * has returned.  The records are those of the contigs the job simulates, in FASTA order: a contig dwgsim_core passes over (DWGSIM_HIP_SKIP_*) has
 * none, as it has no mutations and no reads.  Made by the first device alone; independent of -M.  A non-zero return fails the job.  width as for
 * dwgsim_hip_haplotype_fasta.  To be called before dwgsim_hip_job_prepare / the first contig: DWGSIM_HIP_ERR_STATE later; fn == NULL: off. */
typedef int (*dwgsim_hip_job_haplotype_fn)(void *user, int hap, const void *data, size_t len);
/* devices == NULL or n_devices <= 0: every HIP device the process sees.  options == NULL: GPU gzip, defaults. */
dwgsim_hip_job_t *dwgsim_hip_job_create(const dwgsim_hip_params_t *p, const int *devices, int n_devices, const dwgsim_hip_job_sink_t *sink,
                                        const dwgsim_hip_job_options_t *options, int *err);
/* contigs_add() (dwgsim.c:465-478): every contig of the FASTA (or of its .fai) -- fixes tot_len and n_ref, and is what -m/-b/-v/-x files are
 * checked against.  Then, optionally, regions_bed_init() / muts_input_init() (dwgsim.c:494-506). */
int dwgsim_hip_job_set_contig_table(dwgsim_hip_job_t *job, const char *const *names, const int64_t *lens, int n);
int dwgsim_hip_job_set_regions(dwgsim_hip_job_t *job, const char *path);
int dwgsim_hip_job_set_mutation_input(dwgsim_hip_job_t *job, int type, const char *path);
int dwgsim_hip_job_set_haplotype_sink(dwgsim_hip_job_t *job, dwgsim_hip_job_haplotype_fn fn, void *user, int width);
/* (ABI 8) The truth SAM (dwgsim_hip_set_truth_sam) through the job: once switched on, the records arrive through the sink's reads / reads_at callbacks as
 * stream DWGSIM_HIP_STREAM_SAM, exactly like a FASTQ stream -- a delivery thread of its own, pieces in file order (or with their offsets), gzip members or text as the
 * job's gzip option says.  The header is not part of the stream (dwgsim_hip_truth_sam_header).  -M 2 makes no reads and no SAM.  To be called before
 * dwgsim_hip_job_prepare / the first contig: DWGSIM_HIP_ERR_STATE later; DWGSIM_HIP_ERR_UNSUP for -c 1 / -c 2. */
int dwgsim_hip_job_set_truth_sam(dwgsim_hip_job_t *job, int on);
/* (ABI 9) ... with NM:i: and MD:Z: on its mapped records (dwgsim_hip_set_truth_md).  Before dwgsim_hip_job_prepare / the first contig, like the call above; without
 * it, it does nothing. */
int dwgsim_hip_job_set_truth_md(dwgsim_hip_job_t *job, int on);
/* (ABI 10) The truth VCF (dwgsim_hip_set_truth_depth) through the job.  Every device counts the batches it simulates; when the last batch of a group has been
 * simulated the job fetches the counters of every device that took part, adds them up on the host and calls fn with the records of each of the group's contigs
 * (dwgsim_hip_mutlist_truth_vcf_text; no header: dwgsim_hip_truth_vcf_header), contigs in FASTA order, from ONE thread of the job.  A contig dwgsim_core passes
 * over has none.  Independent of -M (with -M 2 no read is made and every depth is 0).  A non-zero return fails the job.  To be called before
 * dwgsim_hip_job_prepare / the first contig: DWGSIM_HIP_ERR_STATE later; DWGSIM_HIP_ERR_UNSUP for -c 1 / -c 2; fn == NULL: off. */
typedef int (*dwgsim_hip_job_truth_vcf_fn)(void *user, const char *contig, const char *vcf, size_t vcf_len);
int dwgsim_hip_job_set_truth_vcf_sink(dwgsim_hip_job_t *job, dwgsim_hip_job_truth_vcf_fn fn, void *user);
/* (ABI 11) The chain files (dwgsim_hip_haplotype_chain) through the job.  Right behind a group's walk the first device finds the blocks of both haplotypes,
 * and fn gets, for haplotype 0 and then 1, for direction DWGSIM_HIP_CHAIN_TO_REF and then _FROM_REF, the chains of the group's contigs in FASTA order
 * (dwgsim_hip_chain_format) as one piece of the file (hap, direction): the pieces of a file arrive in file order, from ONE thread of the job.  The ids of a
 * file run 1, 2, ... across the groups.  A contig dwgsim_core passes over has no chain, and neither has a haplotype of a contig without an aligned cell.
 * Independent of -M and of the haplotype sink.  A non-zero return fails the job.  To be called before dwgsim_hip_job_prepare / the first contig:
 * DWGSIM_HIP_ERR_STATE later; fn == NULL: off. */
typedef int (*dwgsim_hip_job_chain_fn)(void *user, int hap, int direction, const void *data, size_t len);
int dwgsim_hip_job_set_chain_sink(dwgsim_hip_job_t *job, dwgsim_hip_job_chain_fn fn, void *user);
/* optional: parse the files above and start the device threads now (errors of -x / -m / -b / -v surface here instead of at the first contig) */
int dwgsim_hip_job_prepare(dwgsim_hip_job_t *job, uint64_t *total_len);
/* The body of the contig loop (dwgsim.c:519-625 and everything below it) for the next contig of the FASTA.  Returns the pairs scheduled for
 * it (>= 0), or why it is skipped (DWGSIM_HIP_SKIP_*: test with DWGSIM_HIP_IS_SKIP), or an error code (DWGSIM_HIP_ERR_*: the job has failed, stop
 * feeding it and call finish / last_error).
 * The sequence is copied: `ascii` is the caller's again when the call returns.  Blocks only when the devices are two groups behind. */
int64_t dwgsim_hip_job_add_contig(dwgsim_hip_job_t *job, const char *name, const uint8_t *ascii, int64_t len);
/* The same in two halves, for a caller that produces the sequence itself (seq_read_fasta, mut.c:49-87, with as many threads as it likes):
 * begin returns where the contig's `len` sequence characters go -- page-locked staging of the job, already in the layout the upload needs, so
 * nothing is copied again -- or NULL with *status = an error code; any threads of the caller fill [p, p + len); commit schedules the contig and
 * returns what dwgsim_hip_job_add_contig returns; cancel hands the reservation back (e.g. the record turned out to have another length).  One
 * contig can be open at a time; the pointer is valid until commit / cancel.  begin blocks only when the devices are two groups behind. */
uint8_t *dwgsim_hip_job_begin_contig(dwgsim_hip_job_t *job, const char *name, int64_t len, int64_t *status);
int64_t dwgsim_hip_job_commit_contig(dwgsim_hip_job_t *job);
int dwgsim_hip_job_cancel_contig(dwgsim_hip_job_t *job);
/* no more contigs: returns when everything has been delivered to the sink (DWGSIM_HIP_OK) or the job failed */
int dwgsim_hip_job_finish(dwgsim_hip_job_t *job);
const char *dwgsim_hip_job_last_error(const dwgsim_hip_job_t *job);
void dwgsim_hip_job_destroy(dwgsim_hip_job_t *job);

/* ====================================================================================================================================
 * dwgsim_eval: score SAM or BAM alignments of simulated reads (reference src/dwgsim_eval.c; DESIGN.md "dwgsim_eval-hip").
 * A context evaluates one run: header(file 1), feed(records of file 1)..., header(file 2), feed..., finish, then the texts.  One device.
 * A BAM file is bam_begin, feed_bam(its raw bytes)... instead of header, feed...; SAM and BAM files may be mixed in one run.
 * (ABI 3) A truth SAM, given before the first file (truth_header, truth_feed..., truth_commit), adds a base-level section: every aligned record
 * is joined with its truth record on the device and the two CIGARs are walked side by side (truth_text; the rule: dw_eval.hpp TRUTH).
 * ==================================================================================================================================== */
#define DWGSIM_HIP_EVAL_ABI_VERSION 3
/* fatal record errors (dwgsim_hip_eval_summary_t.error_code): the first record of the run, in file order, that has one decides */
#define DWGSIM_HIP_EVAL_E_MALFORMED       1   /* not a SAM record (fewer than 11 fields, FLAG / POS / MAPQ out of range, ...) */
#define DWGSIM_HIP_EVAL_E_PREFIX          2   /* "could not match read name with given read name prefix (-P)" */
#define DWGSIM_HIP_EVAL_E_NAME            3   /* "read was not generated by dwgsim?" */
#define DWGSIM_HIP_EVAL_E_CONTIG          4   /* "the mapped contig does not exist in the SAM header" */
#define DWGSIM_HIP_EVAL_E_RANDOM_CORRECT  5   /* "predicted value cannot be mapped correctly when the read is unmappable" */
#define DWGSIM_HIP_EVAL_E_PAIRED          6   /* -z: "Found a read that was paired end" */
#define DWGSIM_HIP_EVAL_E_NOT_PAIRED      7   /* no -z: "Found a read that was not paired" */
#define DWGSIM_HIP_EVAL_STOPPED           1   /* dwgsim_hip_eval_feed: a fatal record was found, the rest of the input is not needed */

typedef struct dwgsim_hip_eval_ctx dwgsim_hip_eval_ctx_t;

/* the options of dwgsim_eval (getopt "a:d:e:g:m:n:q:s:bchimpzSP:"), defaults from dwgsim_hip_eval_opts_default */
typedef struct dwgsim_hip_eval_opts {
    uint32_t size;                  /* sizeof(dwgsim_hip_eval_opts_t) */
    int32_t a, d, e, g, n, q, s;    /* -a 0, -d 1 (not 0), -e -1, -g 5, -n 0, -q 0, -s -1 */
    int32_t b, c, i, m, p, z;       /* flags, 0 */
    const char *P;                  /* -P, NULL: none (copied at create) */
    uint64_t chunk_bytes;           /* text per device chunk; 0: 32 MiB.  At least 4 KiB */
    int32_t inflate_threads;        /* (ABI 2) host threads that inflate BGZF blocks; 0: 8.  At most 16; 1: the calling thread alone */
} dwgsim_hip_eval_opts_t;

typedef struct dwgsim_hip_eval_summary {
    uint32_t size;                  /* sizeof(dwgsim_hip_eval_summary_t), set by the caller */
    int32_t status;                 /* the exit status of dwgsim_eval: 0, or 1 after a fatal record error */
    int32_t error_code;             /* DWGSIM_HIP_EVAL_E_*, 0 */
    int32_t reserved;
    uint64_t error_record;          /* 0-based index of that record among the record lines of the run */
    uint64_t n;                     /* pairs (single-end reads with -z) */
    uint64_t records;               /* record lines evaluated */
    const char *stderr_text;        /* what dwgsim_eval writes to stderr (fatal error, -n warning, "Analysis complete."); valid until destroy */
    size_t stderr_len;
} dwgsim_hip_eval_summary_t;

void dwgsim_hip_eval_opts_default(dwgsim_hip_eval_opts_t *opts);
/* *err: DWGSIM_HIP_OK, DWGSIM_HIP_ERR_ARG (size, -d 0, chunk), DWGSIM_HIP_ERR_DEVICE */
dwgsim_hip_eval_ctx_t *dwgsim_hip_eval_create(const dwgsim_hip_eval_opts_t *opts, int device, int *err);
/* starts the next file: its header text (the '@' lines; the @SQ SN: names are its targets) */
int dwgsim_hip_eval_header(dwgsim_hip_eval_ctx_t *ctx, const char *text, size_t len);
/* record text of the current file, split anywhere.  DWGSIM_HIP_EVAL_STOPPED once a fatal record has been found */
int dwgsim_hip_eval_feed(dwgsim_hip_eval_ctx_t *ctx, const char *buf, size_t len);
/* starts the next file, a BAM file (and ends the file before it, as dwgsim_hip_eval_header does): its targets are its binary reference list */
int dwgsim_hip_eval_bam_begin(dwgsim_hip_eval_ctx_t *ctx);
/* raw bytes of the current BAM file (BGZF), split anywhere.  DWGSIM_HIP_EVAL_STOPPED as for feed.  A container error (not BGZF, inflate,
 * CRC-32 or ISIZE mismatch, bad BAM magic or header, and -- at the next begin / header / finish -- a file that ends inside a block, the
 * header or a record) is DWGSIM_HIP_ERR_FAILED once the records in front of it hold no fatal one; last_error says what and where */
int dwgsim_hip_eval_feed_bam(dwgsim_hip_eval_ctx_t *ctx, const void *buf, size_t len);
int dwgsim_hip_eval_finish(dwgsim_hip_eval_ctx_t *ctx, dwgsim_hip_eval_summary_t *summary);
/* after finish without a fatal error: the 19 '#' lines and the rows (stdout of dwgsim_eval after the -p part) */
int dwgsim_hip_eval_table_text(dwgsim_hip_eval_ctx_t *ctx, const char **txt, size_t *len);
/* with -p: the first file's header and the incorrectly mapped records, verbatim, in input order */
int dwgsim_hip_eval_incorrect_text(dwgsim_hip_eval_ctx_t *ctx, const char **txt, size_t *len);
/* Breakdown: the table of every stratum of the chosen dimensions, computed in the same pass as the main table (off by default).
 * dims: a comma list of snps (n_sub_1, as -s), errors (n_err_1, as -e), indels (the record's own end, as -i), end (first / second end); NULL or
 * empty: off.  cap: snps and errors have the strata 0 ... cap-1 and cap+ (everything else, negative values too); 0: 8, at most 32.  A record that
 * enters the main table is counted in one stratum of every dimension, so "snps=k" is the table of a run with -s k.  To be called after create and
 * before the first header / bam_begin / feed: DWGSIM_HIP_ERR_STATE later; DWGSIM_HIP_ERR_ARG for an unknown or repeated name or a cap outside 0 ... 32. */
int dwgsim_hip_eval_set_breakdown(dwgsim_hip_eval_ctx_t *ctx, const char *dims, int cap);
/* after finish: empty when the breakdown is off or the run ended in a fatal record, else one section per stratum -- the line "## snps=0\n"
 * ("## snps=8+", "## errors=3", "## indels=0", "## indels=1+", "## end=1", "## end=2") and that stratum's table as in table_text -- in the order
 * snps, errors, indels, end, strata ascending, empty strata included (the one-row-of-zeros table) */
int dwgsim_hip_eval_breakdown_text(dwgsim_hip_eval_ctx_t *ctx, const char **txt, size_t *len);
/* Truth (ABI 3): the true alignment of every read end, as dwgsim-hip writes it (out.truth.sam).  All four calls below but truth_text are legal
 * only after create and before the first header / bam_begin / feed: DWGSIM_HIP_ERR_STATE later, and a context whose truth is not committed
 * refuses header / bam_begin / feed with DWGSIM_HIP_ERR_STATE; so does truth_header once truth_feed has been called.  A truth and a breakdown in one context: DWGSIM_HIP_ERR_ARG and a message.
 * truth_header: the truth SAM's '@' lines; their @SQ SN: names are the truth's contigs (an aligned record has the truth's contig when its
 *   RNAME -- through the targets of its own file -- is the same name).
 * truth_feed: record text, split anywhere, any number of calls.  A key is (QNAME, end): end 0 when FLAG 0x1 is clear, else (FLAG >> 6) & 3.
 *   DWGSIM_HIP_ERR_FAILED and "truth: record line N ..." (N counts record lines from 1) for a line with fewer than 11 fields, one that is no
 *   truth record (QNAME, FLAG, POS, end 3 or a paired end 0), a mapped line at POS 0, with an RNAME outside the @SQ names, or with a CIGAR
 *   that is no sequence of M, I and D runs with at least one query base; DWGSIM_HIP_ERR_NOMEM when the truth does not fit in device memory; DWGSIM_HIP_ERR_ARG for more
 *   than 2^32 - 2 records.  After such an error the truth calls return DWGSIM_HIP_ERR_FAILED.
 * truth_commit: builds the index and returns when it is complete and every record has found itself in it.  Two records with one key fail it:
 *   DWGSIM_HIP_ERR_FAILED, "truth: the truth holds read of record line N twice (... record line M)".
 * truth_text: after finish.  Empty without a truth or after a fatal record; else, for the strata all and indel (truth CIGARs with an I or a D),
 *   "## truth all" / "## truth indel", a '#' line naming the columns, and one tab-separated row per MAPQ value that a record of the stratum
 *   has, highest first, counts cumulative over MAPQ >= the row's: mapq missing random unusable compared exact bases right clipped ibases
 *   iright.  A stratum without records has one row of zeros at MAPQ 0.  The main table, -p text and stderr are those of a run without a truth. */
int dwgsim_hip_eval_truth_header(dwgsim_hip_eval_ctx_t *ctx, const char *text, size_t len);
int dwgsim_hip_eval_truth_feed(dwgsim_hip_eval_ctx_t *ctx, const char *buf, size_t len);
int dwgsim_hip_eval_truth_commit(dwgsim_hip_eval_ctx_t *ctx);
int dwgsim_hip_eval_truth_text(dwgsim_hip_eval_ctx_t *ctx, const char **txt, size_t *len);
const char *dwgsim_hip_eval_last_error(const dwgsim_hip_eval_ctx_t *ctx);
void dwgsim_hip_eval_destroy(dwgsim_hip_eval_ctx_t *ctx);
/* test hooks: the device time (ms, HIP events) of the chunks so far; and kernel-only throughput: `len` bytes of record lines (host memory)
 * are uploaded once and then evaluated `reps` times as one chunk from device memory, *ms = time per evaluation.  The run's counts are untouched
 * except for the histogram, which this adds to.  With a breakdown set, both device_chunk hooks run the breakdown form of the record kernel. */
int dwgsim_hip_eval_debug_time(dwgsim_hip_eval_ctx_t *ctx, double *kernel_ms);
int dwgsim_hip_eval_debug_device_chunk(dwgsim_hip_eval_ctx_t *ctx, const void *text, size_t len, int reps, double *ms);
/* the same for a BAM chunk: `len` bytes of whole BAM records (uncompressed, no header; the targets are those of the context's current BAM
 * file), k_eval_bam_records alone, *ms = time per evaluation.  And the inflater alone, without a device: all BGZF blocks of the `len` bytes of a
 * BAM file on `threads` host threads, *ms = the best of `reps` passes, *out_bytes = the inflated size. */
int dwgsim_hip_eval_debug_device_bam_chunk(dwgsim_hip_eval_ctx_t *ctx, const void *records, size_t len, int reps, double *ms);
int dwgsim_hip_eval_debug_inflate(const void *bam, size_t len, int threads, int reps, double *ms, uint64_t *out_bytes);
/* before truth_commit: the index gets 2^log2_slots slots instead of at least twice the records (more slots than records, or commit fails with
 * DWGSIM_HIP_ERR_ARG): a nearly full table, whose probe chains are long and wrap around its end.  With a truth, the device_chunk hooks run the
 * truth form of the record kernels. */
int dwgsim_hip_eval_debug_truth_slots(dwgsim_hip_eval_ctx_t *ctx, int log2_slots);

/* ====================================================================================================================================
 * TEST / ANALYSIS HOOKS -- everything below this line is NOT part of the drop-in surface.  A binding of the reference needs none of it; the
 * parity tests and the profiling scripts do.  (All of it is read-only with respect to what the product computes: the options select between
 * code paths that produce the same bytes, the self-tests and counters only report.)
 * ==================================================================================================================================== */
/* "justify_seq" = 1: left-justification from one thread (cross-check of the cluster-parallel form); "walk_cap" = n: start the mutation walk with
 * room for n candidates (exercises the exact re-run); "walk_seg_min" = n: segmented form of the walk's serial scans from n candidates on;
 * "writer" = 0 / 1: force the register / LDS-FIFO record writer; "sim_threads" = 64 / 256: force the one-wave blocks of the long-read variant / the 256-lane blocks (where their reads fit LDS);
 * "place_cap" = n: room for n undecided pairs per list in dwgsim_hip_count_random* (exercises its second run); "split" = 0 / 1: the Illumina
 * read kernel as one kernel with look-backs / as two kernels with the offsets computed in between (default: two for reads of up to 100 bases); "qrows" = 0: the quality line of
 * the single Illumina kernel stays on the per-lane FIFO where it would run in the wave's staging rows (reads of 137 bases on); "flow_slots" = n:
 * n scratch slots per XCD for the Ion Torrent read buffers / the long reads of the one-wave blocks (blocks wait for slots); "flow_cap" = n: the Ion Torrent
 * read capacity a job starts from (a read that outgrows it makes the batch run again with twice the room); "phases" = 1: print the phase
 * split of the -DDW_PHASE_TIMING analysis build; "truth_cap" = n: the bytes a batch's tagged truth SAM (dwgsim_hip_set_truth_md) is planned with at first
 * (exercises the second run that finds the room). */
int dwgsim_hip_debug_option(dwgsim_hip_ctx_t *ctx, const char *key, int64_t value);
/* "place_open": pairs the last dwgsim_hip_count_random* call could not settle from the coarse haplotype summaries; "flow_cap_mult": how often (as a
 * power of two) the Ion Torrent read capacity has been doubled so far; "walk_us" / "count_us":
 * HIP-event time (microseconds, accumulated) of the context's walk chains / random-read counts on the walk stream; "sim_form": the
 * k_simulate<LPP, OUT, DT, NTHR, WR, SPLIT> form of the context's last simulate launch (0 before the first), packed as
 * NTHR << 20 | LPP << 16 | OUT << 12 | DT << 8 | WR << 4 | SPLIT (SPLIT 1: the two-kernel form, WR: the writer of its second half); "walk_form": what
 * the context's last mutation walk enqueued was made of (0 before the first), packed as ATTEMPT << 16 | FILE << 12 | SLOTS << 8 | RESTORE << 4 | DENSE
 * (ATTEMPT 1, 2: the exact re-runs; FILE 1: the file-driven walk of -m / -b / -v; SLOTS 1 / 0: the slot / look-back form of the site scan; RESTORE: what
 * went back to the pristine copies first -- 0 nothing, 1 the dirty chunks, 2 whole buffers; DENSE 1 / 0: views made from every cell / from the dirty bitmap);
 * "hap_len_us" / "hap_write_us": HIP-event time (microseconds) of the length pass + scan / of the header and write kernels of the haplotype text built
 * last (dwgsim_hip_haplotype_fasta); "hap_copy_us": with the option "hap_yardstick" = 1, of a device-to-device copy of that text's size behind it;
 * "truth_us": HIP-event time (microseconds) of the truth step of the batch waited for last (dwgsim_hip_set_truth_sam); "truth_copy_us": of the device-to-device copy
 * of n bytes of slot 0's truth SAM that the option "truth_yardstick" = n makes at once; "truth_reruns": batches of the context that ran a second time because
 * their tagged truth SAM needed more room than planned; "chain_count_us" / "chain_write_us": HIP-event time (microseconds) of the count pass + scan / of the
 * write pass of the chain built last (dwgsim_hip_haplotype_chain), "chain_blocks": the blocks of the group it built or found */
int dwgsim_hip_debug_get(dwgsim_hip_ctx_t *ctx, const char *key, int64_t *value);
/* (ABI 9) the two calls above through a job: the option goes to every context of the job (before dwgsim_hip_job_prepare / the first contig: DWGSIM_HIP_ERR_STATE
 * later); the value is the sum over the job's contexts (before the first contig or after dwgsim_hip_job_finish).  dwgsim-hip: DWGSIM_HIP_DEBUG="key=value,..."
 * sets the options and makes the program report "truth_reruns" on stderr. */
int dwgsim_hip_job_debug_option(dwgsim_hip_job_t *job, const char *key, int64_t value);
int dwgsim_hip_job_debug_get(dwgsim_hip_job_t *job, const char *key, int64_t *value);
/* (ABI 7) the k_simulate<LPP, OUT, DT, NTHR, WR, SPLIT> instances the library was built with, from the list that instantiates them and in which a
 * launch looks its form up: returns their number and writes at most `cap` of them to `out` (may be NULL), each packed as "sim_form" above with SPLIT
 * the template parameter -- 0: the single kernel, 1 / 2: the first / second half of the two-kernel form.  A form with SPLIT 1 that "sim_form" reports,
 * (l, o, d, n, w, 1), runs the instances (l, 1, d, n, 1, 1) and (l, o, d, n, w, 2).  Needs no context and no device. */
int dwgsim_hip_debug_sim_instances(int64_t *out, int cap);
/* the gzip kernel on arbitrary host bytes (the product only ever feeds it FASTQ text) */
int dwgsim_hip_debug_gzip(dwgsim_hip_ctx_t *ctx, const void *text, size_t n, void *out, size_t cap, size_t *out_n);
/* occurrences of `byte` in one finished stream of a slot, counted on the device (whole-output checks without a copy-out) */
int dwgsim_hip_debug_count_byte(dwgsim_hip_ctx_t *ctx, int slot, int stream, int byte, uint64_t *count);
/* device self-tests of the arithmetic shortcuts (dw_common.hpp / dw_simulate.hip): the range-restricted fp64 division / sqrt / log against the
 * compiler's general forms on n operand sets; the lazy fp32 quality normals against the exact fp64 form on n tries from `first` (n = 2^32: every
 * try) and, with exhaustive != 0, the hardware log2 / rcp / sqrt on every float of their operand ranges.  out: see dw_host.cpp. */
int dwgsim_hip_selftest_fp64(int device, uint32_t seed, uint64_t n, uint64_t *out);
int dwgsim_hip_selftest_lazy(int device, uint32_t first, uint64_t n, double sigma, int exhaustive, uint64_t *out);
/* the number formatters of the name line (decimal positions and counts, the hexadecimal read index: dw_read.hpp put_dec / put_hex) against one
 * division per digit on the values first + i * stride, i < n.  out[0] / out[1]: decimal / hexadecimal texts that differ, out[2]: values compared. */
int dwgsim_hip_selftest_text(int device, uint64_t first, uint64_t n, uint64_t stride, uint64_t *out);
/* the gap draw of the error sites, walk sites and flow first draws (dw_common.hpp geom_gap) at threshold thr (0 < thr < 2^32), with the product's own
 * table and reciprocal, on the words [first, first + n).  chg[k] (g_cnt words): the first word of the range whose gap is below g_lo + k (0: none);
 * out[0]: words where the gap increases with the word, out[1]: words at the clip 0x3FFFFFFF, out[2]: words evaluated, out[3]: the gap of the last word. */
int dwgsim_hip_selftest_gap(int device, uint64_t thr, uint32_t first, uint64_t n, uint32_t g_lo, uint32_t g_cnt, uint32_t *chg, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif
