/*
 * kmerpapa_hip.h -- C-ABI of the MI355X lattice-DP engine (libkmerpapa_hip.so).
 *
 * Plain C types only (no torch, no HIP types).  Every call returns KP_OK (0) or a
 * negative KP_E_* code; kp_last_error() gives the thread's last message.  Host buffers
 * are owned by the caller and only read (or written, for outputs) during the call.
 * Device memory is owned by the plan and cached across passes.
 *
 * What each entry point replaces in the reference (BesenbacherLab/kmerPaPa v0.2.4;
 * "CV" = src/kmerpapa/algorithms/bottum_up_array_penalty_plus_pseudo_CV.py,
 *  "Fit" = src/kmerpapa/algorithms/bottum_up_array_w_numba.py):
 *
 *   kp_plan_create   per-pattern globals and tables: CV :82-122, Fit :68-92;
 *                    pattern_utils.py pattern_max :587, get_cum_genpat_pos_level :237,
 *                    subpatterns_level_ord_np :513 (level order)
 *   kp_set_counts    level-0 rows of M_mem/U_mem written by
 *                    CV_tools.make_all_folds_contextD_patterns (CV :130) or by the Fit
 *                    level-0 loop (Fit :106-114), plus every aggregated row
 *                    (first-pair sums, CV :52-55 / Fit :50-53)
 *   kp_pass          the level sweep CV :143-157 (score_test_folds :15-20 and
 *                    handle_pattern :26-78 for every cell) and its root read-out
 *                    :158-163; with fold = -1 the Fit sweep Fit :106-120
 *   kp_fit_leaves    backtrack(gen_pat, ...) Fit :17-24, 121
 *   kp_counts_begin / kp_counts_fold   the same, one fold at a time
 *   kp_fold_split    CV_tools.py sample :5-27 and the fold loop of
 *                    make_all_folds_contextD_patterns :44-57 (host code, numpy legacy RNG);
 *                    kp_fold_sample: one fold of it (sample :5-27)
 *   kp_kmer_parse    io_utils.py read_dict :82-136 (with downsize_contextD's centring,
 *                    :50-79) and read_joint_kmer_counts :3-46 (host code)
 *   kp_format_long_rows  the -l rows of cli.py:301-316 (host code)
 *   kp_greedy        greedy_penalty_plus_pseudo.py: greedy_res_kmer_table_ord :159-196 with
 *                    train_loss :18-25 per lane, and the test terms of
 *                    CrossValidation.loglik :324-334 (test_logLik :28-35) per chain
 *   kp_apply         papa.PatternPartition's checks (papa.py:53-107, with the pairwise one it
 *                    leaves commented out) and get_M_U (pattern_utils.py:192-215) for every
 *                    pattern of a partition over any table, by mask matching
 *   kp_seq_*         nothing: the reference starts from count files and its README names an
 *                    external tool (kmer_counter snv / background) for producing them
 *   kp_pred_*        nothing: taking a fitted partition's rates back to the positions and
 *                    regions of a genome
 *   kp_spec_*, kp_seq_*_typed   nothing: the same two steps for every mutation type at once
 */
#ifndef KMERPAPA_HIP_H
#define KMERPAPA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KP_OK 0
#define KP_E_ARG (-1)     /* bad argument (pattern, sizes, lane count)            */
#define KP_E_NOMEM (-2)   /* lattice x lanes does not fit device memory             */
#define KP_E_HIP (-3)     /* HIP runtime / launch failure                           */
#define KP_E_STATE (-4)   /* call order violated (e.g. kp_pass before kp_set_counts) */
#define KP_E_PARITY (-5)  /* internal consistency check failed (argmin tree broken) */

#define KP_GROUP_MAX_LANES 8

typedef struct kp_ctx kp_ctx;
typedef struct kp_plan kp_plan;

/* One (pseudo-count alpha, fold) group: n_lanes penalties share the fold's counts.
 * fold in [0, nf) = cross-validation on that fold (train = all other folds);
 * fold = -1      = fit on all data (the Fit module's DP). */
typedef struct {
    int32_t fold;
    int32_t n_lanes;
    double alpha;
    double beta;
    double penalty[KP_GROUP_MAX_LANES];
} kp_group;

typedef struct {
    uint64_t npat;        /* lattice cells = pattern_max(gen_pat)                  */
    uint64_t nblocks;     /* LDS blocks                                            */
    uint64_t n_kmers;     /* k-mers matching gen_pat                               */
    uint32_t block;       /* cells per block (low positions)                       */
    uint32_t block_pad;   /* row stride of a block lane                            */
    int32_t k, low_positions, max_level, high_levels;
    double pairs_total;   /* split pairs summed over all cells (SURVEY 8d "P")    */
    double pairs_high;    /* ... of which at high (gathered) positions             */
    uint64_t bytes_per_lane; /* device bytes per lane: f32 train score per cell
                                (value-only sweep) + backtrack node pool + leaves */
    uint32_t lanes_per_workgroup; /* lanes one sweep workgroup holds at the plan's count
                                     width (32-bit until counts are set): passes cut
                                     into pieces of this width run best */
    uint32_t pad_;
} kp_plan_info;

typedef struct {
    double dp_ms;         /* device time of the DP sweep kernels (HIP events)      */
    double backtrack_ms;  /* device time of the backtrack kernel                   */
    double total_ms;      /* host wall time of the whole kp_pass call              */
    uint64_t units;       /* cells x lanes scored in the pass                      */
    uint64_t dp_launches; /* kernel launches of the sweep                          */
    double alg_bytes;     /* algorithmic bytes of the pass (SURVEY 8d definition)  */
    double gather_bytes;  /* bytes the sweep gathers from HBM/L2 (high splits)     */
} kp_pass_stats;

const char *kp_last_error(void);
int kp_device_count(int *n);

int kp_create(int device, kp_ctx **out);
void kp_destroy(kp_ctx *ctx);
/* free / total device memory of the context's GPU (bytes) */
int kp_device_mem(kp_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* max_block = 0 -> default LDS block budget (4096 cells). */
int kp_plan_create(kp_ctx *ctx, const char *gen_pat, uint32_t max_block, kp_plan **out);
void kp_plan_destroy(kp_plan *plan);
int kp_plan_get_info(const kp_plan *plan, kp_plan_info *out);
/* Host-only (no GPU): build the plan's tables on the host and report their info -- the
 * lattice size and device bytes per lane a job would need, before any device is touched. */
int kp_plan_host(const char *gen_pat, uint32_t max_block, kp_plan_info *out);
/* The same at count width itype_bytes (4 or 8, CV :94-97's itype): lanes_per_workgroup is
 * then the width kp_pass cuts device groups by on an MI355X (160 KiB of LDS per CU), the
 * group size a multi-GPU job deals whole to its ranks. */
int kp_plan_host_counts(const char *gen_pat, uint32_t max_block, int itype_bytes, kp_plan_info *out);
/* Checks of the block list (test hooks; no reference counterpart).  The device builds the
 * plan's block list (blocks by high level) from a closed-form rank rule.
 * kp_block_order_check, host-only: *mismatches = blocks whose closed-form slot differs from
 * the host's block walk.  kp_plan_block_check: *mismatches = entries of the plan's device
 * list that differ from the host walk.  kp_block_list_host, host-only: the host walk's
 * list itself, hlist[nblocks] (blocks in list order) and the level offsets
 * hoff[high_levels + 1] into it (either may be null). */
int kp_block_order_check(const char *gen_pat, uint32_t max_block, uint64_t *mismatches);
int kp_plan_block_check(kp_plan *plan, uint64_t *mismatches);
int kp_block_list_host(const char *gen_pat, uint32_t max_block, uint32_t *hlist, uint64_t *hoff);

/* Upload fold counts of every k-mer: M, U are [n_kmers][nf] arrays of itype_bytes (4 or
 * 8) unsigned integers, k-mers in KmerEnumeration order (position 0 fastest, nucleotide
 * index = position in code[g]).  Builds the per-block k-mer-low count tables. */
int kp_set_counts(kp_plan *plan, const void *M, const void *U, uint64_t n_kmers, int nf, int itype_bytes);

/* The same tables fold by fold, so that passes can start while the host still draws the
 * later folds (the CV driver's pipelined fold split).  kp_counts_begin: M_all, U_all
 * [n_kmers] = counts of all data (the sum of the folds to come; the train counts of fold f
 * are all data minus fold f, CV :22-24); it discards any fold set before.
 * kp_counts_fold: M_fold, U_fold [n_kmers] = fold `fold`'s counts; asynchronous (the
 * counts are copied before it returns, the table fills on the plan's count stream, and
 * every later device read of it waits for that on the device), so it may be called from
 * another host thread while a kp_pass of another fold runs.  kp_pass refuses a group
 * whose fold has not been set (KP_E_STATE). */
int kp_counts_begin(kp_plan *plan, const void *M_all, const void *U_all, uint64_t n_kmers, int nf, int itype_bytes);
int kp_counts_fold(kp_plan *plan, int fold, const void *M_fold, const void *U_fold, uint64_t n_kmers);

/* One DP sweep of every lane of every group over the whole lattice.
 * Lanes are numbered group-major; per lane the outputs are the root's train score
 * (f32, as stored by the reference), the root's test -2LL (CV) and the number of
 * patterns of the optimal partition. */
int kp_pass(kp_plan *plan, const kp_group *groups, int n_groups, float *root_train, float *root_test,
            uint64_t *n_leaves);
int kp_last_pass_stats(const kp_plan *plan, kp_pass_stats *out);
/* Host-only (no GPU): the workgroups ("device groups") kp_pass would run `groups` as, with
 * `lanes_per_workgroup` lanes per workgroup (kp_plan_info): lane0[i] / nl[i] = first lane
 * and lanes of device group i (lanes numbered group-major), nl2[i] = its trailing lanes
 * that take a second (alpha, beta) (a mixed group of two same-fold groups; 0 = one alpha).
 * *n_out = number of device groups; at most cap entries are written. */
int kp_device_groups(const kp_group *groups, int n_groups, int lanes_per_workgroup, int32_t *lane0, int32_t *nl,
                     int32_t *nl2, int cap, int *n_out);
/* Tuning: with KP_LAUNCH_TIMES=1 in the environment, the device time (ms) of every sweep
 * launch of the last pass (lane classes in order, high levels ascending); *n = launches
 * (0 without the variable), at most cap written to ms. */
int kp_last_launch_ms(const kp_plan *plan, float *ms, int cap, int *n);

/* Allocate the per-lane device buffers (score rows, backtrack nodes) for `lanes` lanes now,
 * so that later passes of up to that many lanes allocate nothing.  Buffers only grow.
 * Re-allocating after a free is slow on MI355X (freed HBM is wiped first), so a job that
 * knows its largest pass should reserve it once.  KP_E_NOMEM if it does not fit.
 * (No reference counterpart: the reference allocates its [npat, nf] arrays per call, CV
 * :93-102.) */
int kp_reserve_lanes(kp_plan *plan, uint32_t lanes);

/* Leaves (cell indices) of lane `lane` of the last pass, in the reference's backtrack
 * order.  cap = capacity of `leaves`; *n_out = number of leaves. */
int kp_fit_leaves(kp_plan *plan, uint32_t lane, uint64_t *leaves, uint64_t cap, uint64_t *n_out);

/* Debug / parity: copy one lane's train scores and argmin codes, in cell-index order
 * ([npat] each; either pointer may be NULL). */
int kp_dump_lane(kp_plan *plan, uint32_t lane, float *score, uint8_t *code);

/* Debug / parity: the train scores of the cells cells[0..n) (cell indices < npat) of lane
 * `lane` of the last pass, into out[n] -- e.g. every cell of a sub-pattern embedded in a
 * full-size lattice, whose values depend only on its own sub-lattice. */
int kp_gather_cells(kp_plan *plan, uint32_t lane, const uint64_t *cells, uint64_t n, float *out);

/* Parity check of the device's float64 log (the log of the single-pattern term, CV :61-62 /
 * Fit :56-57; ROCm's ocml): y[i] = log(x[i]) computed on the context's GPU. */
int kp_math_log(kp_ctx *ctx, const double *x, double *y, uint64_t n);

/* Parity check of the C library's log / log1p as restated for the GPU (kp_libm.h: the
 * sweep's exact fallback, the backtrack and the k-mer terms): fn 1 = log, 2 = log1p
 * (fn 0 = the device's own log, as kp_math_log; fn 3 = kp_fast_log, the table-free fdlibm
 * log; fn 4 = kp_fma_log, its FMA / hardware-reciprocal form), computed on the context's GPU. */
int kp_math_libm(kp_ctx *ctx, const double *x, double *y, uint64_t n, int fn);

/* --score all_kmers on the context's GPU: one rate per k-mer, no lattice DP
 * (src/kmerpapa/algorithms/all_kmers_CV.py: test_folds :8-13 and the k-mer loop :36-46).
 * M, U: [n][nf] uint64 fold counts, rows in the reference's matches(gen_pat) order; per
 * alpha a (alphas[na]) and fold f, with betas[a][f] (get_betas of the fold-train totals):
 *   sum_train[a][f] = sum over rows i of test_folds(trM, trU, trM, trU, alpha_a, beta_af)
 *   sum_test[a][f]  = sum over rows i of test_folds(trM, trU, M[i][f], U[i][f], alpha_a, beta_af)
 * trM = sum_g M[i][g] - M[i][f] (likewise trU); each sum in float64, row by row from 0.0,
 * as the reference's `sum_train += ...` loop; xlogy / xlog1py with the C library's logs. */
int kp_allkmers_cv(kp_ctx *ctx, const uint64_t *M, const uint64_t *U, uint64_t n, int nf, const double *alphas,
                   const double *betas, int na, double *sum_train, double *sum_test);

/* The greedy top-down partition (--greedy / --greedyCV;
 * src/kmerpapa/algorithms/greedy_penalty_plus_pseudo.py: train_loss :18-25, test_logLik
 * :28-35, greedy_res_kmer_table_ord :159-196, the loop of CrossValidation.loglik :324-334).
 * No lattice: only the k-mer count table and one tree per lane are on the device.
 * A lane is one tree: fold = -1 grows it on all data, fold f on all data minus fold f (whose
 * counts are then the test counts); chain >= 0 adds the lane's test terms, leaf by leaf in
 * partition order, to chain_test[chain] after those of the earlier lanes of that chain (from
 * 0.0: the reference's `test_ll` of one repeat); chain = -1 adds them nowhere.
 * gen_pat: IUPAC, at most 16 positions (a pattern is a uint64 of 4-bit nucleotide masks,
 * A = 1, C = 2, G = 4, T = 8, position 0 lowest).  M, U: [n_kmers][max(nf, 1)] uint64, rows in
 * matches(gen_pat) order; with nf > 1 the columns are the fold tables and all data is their
 * sum.  Totals of 2^53 or more are KP_E_ARG (the reference sums counts in float64).
 * Outputs per lane: loss[lane] (float64, s1 + s2 along the tree) and n_leaves[lane];
 * chain_test[max chain + 1].  Lanes run in batches that fit free device memory minus 2 GiB
 * (KP_GREEDY_MEM = bytes overrides that budget; KP_GREEDY_CHUNK = k-mers per histogram
 * chunk, default 4096); KP_E_NOMEM if the tables and one lane do not fit. */
typedef struct {
    int32_t fold;
    int32_t chain;
    double alpha;
    double beta;
    double penalty;
} kp_greedy_lane;
int kp_greedy(kp_ctx *ctx, const char *gen_pat, const uint64_t *M, const uint64_t *U, uint64_t n_kmers, int nf,
              const kp_greedy_lane *lanes, int n_lanes, double *loss, double *chain_test, uint64_t *n_leaves);
/* The partition of lane `lane` of the context's last kp_greedy call, in the reference's
 * order (left subtree's patterns first), as pattern words; ctx = NULL: of this thread's
 * last kp_greedy_host call.  cap = capacity of `patterns`; *n_out = number of patterns. */
int kp_greedy_leaves(kp_ctx *ctx, uint32_t lane, uint64_t *patterns, uint64_t cap, uint64_t *n_out);
/* Figures of the context's last kp_greedy call (measurement, tests of the memory budget). */
typedef struct {
    double hist_ms;          /* device time of the histogram kernel, all depths (HIP events) */
    double total_ms;         /* host wall time of the whole call                             */
    uint64_t frontier_kmers; /* k-mers of all frontier nodes, summed over depths and lanes:
                                the rows the histogram kernel read                           */
    uint64_t items;          /* (node, chunk) work items = waves of the histogram kernel     */
    uint32_t depths;         /* levels of the deepest tree                                   */
    uint32_t batches;        /* lane batches the call ran                                    */
} kp_greedy_stats;
int kp_greedy_last_stats(kp_ctx *ctx, kp_greedy_stats *out);
/* Host-only (no GPU): the same call and outputs computed serially on the host with the
 * per-node code the kernels run (parity and CPU tests; not a product path). */
int kp_greedy_host(const char *gen_pat, const uint64_t *M, const uint64_t *U, uint64_t n_kmers, int nf,
                   const kp_greedy_lane *lanes, int n_lanes, double *loss, double *chain_test, uint64_t *n_leaves);

/* A fitted partition applied to a k-mer count table: which pattern each row belongs to, the
 * table's counts per pattern, whether the patterns are a partition at all, and the table's
 * -2 log-likelihood under given rates.  (The reference has papa.PatternPartition's
 * constructor checks, papa.py:53-107 -- its pairwise check is commented out as slow -- and
 * get_M_U, pattern_utils.py:192-215, which enumerates every k-mer of a pattern.)  Nothing is
 * enumerated here: row i matches pattern j when (onehot(codes[i]) & ~patterns[j]) == 0, so the
 * table may be sparse (observed k-mers only) and k may be up to 16.
 * patterns[n_patterns], super_word: pattern words as kp_greedy's (4-bit masks, position 0
 * lowest).  codes[n]: 2 bits per letter, first letter most significant (kp_kmer_parse);
 * M, U: [n][ncol] counts.  Outputs: pid[n] (may be NULL) = the row's pattern, -1 if none
 * matches, -2 if several do; pat_M, pat_U [n_patterns][ncol] = counts of the rows with exactly
 * one match, summed as integers; with rates[n_patterns] (may be NULL, then ll is not written)
 * ll[c] = -2 * sum over patterns, in order from 0.0, of xlogy(pat_M, rate) + xlog1py(pat_U,
 * -rate): score_utils.get_loss with penalty 0, bit for bit.  stats: rows without / with
 * several matches, pattern pairs that share a k-mer, patterns that are not sub-patterns of
 * super_word.  KP_E_ARG: k outside 1..16, a code with bits above 2k, a pattern (or super_word)
 * with an empty position or bits above position k, a negative count, a column total of 2^63
 * or more, n_patterns = 0.  n = 0 is valid.  KP_E_NOMEM if the table does not fit device
 * memory.  Knobs, read at each call (every setting gives the same results): KP_APPLY_TILE =
 * patterns per LDS tile (default 1024; 0 = no tiles, the patterns come through the scalar
 * cache), KP_APPLY_GLOBAL=1 = totals by global atomics, KP_APPLY_LDS=1/0 = totals in LDS
 * counters per workgroup required (KP_E_ARG if they do not fit) / off (default: on when
 * they fit and the workgroups' flushes, workgroups x 2 x n_patterns x ncol, are no more
 * atomics than the 2 x n x ncol of adding directly), KP_APPLY_GRID = most workgroups to
 * launch. */
typedef struct {
    uint64_t unmatched, multi;
    uint64_t overlap_pairs, outside_super;
    double assign_ms;      /* device time of kp_apply_assign (HIP events; 0 on the host)    */
    uint32_t tiles;        /* pattern tiles per row sweep (0 = scalar-cache path, or host)  */
    uint32_t lds_counters; /* 1 = the totals were summed in LDS counters per workgroup      */
} kp_apply_stats;
int kp_apply(kp_ctx *ctx, int k, const uint64_t *patterns, uint32_t n_patterns, uint64_t super_word,
             const uint64_t *codes, const int64_t *M, const int64_t *U, uint64_t n, int ncol, const double *rates,
             int32_t *pid, uint64_t *pat_M, uint64_t *pat_U, double *ll, kp_apply_stats *stats);
/* Host-only (no GPU): the same call run serially on the host by the same per-row / per-pair /
 * per-term code (parity and CPU tests; not a product path). */
int kp_apply_host(int k, const uint64_t *patterns, uint32_t n_patterns, uint64_t super_word, const uint64_t *codes,
                  const int64_t *M, const int64_t *U, uint64_t n, int ncol, const double *rates, int32_t *pid,
                  uint64_t *pat_M, uint64_t *pat_U, double *ll, kp_apply_stats *stats);

/* k-mer context counts of a genome and of its mutation sites: the two count tables every other
 * entry point starts from.  (No reference counterpart: the reference's README names an
 * external tool, kmer_counter, for this step; the semantics below are this project's own.)
 * A contig is an array of bytes, one per base: A, C, G, T in either case are bases, every other
 * byte is invalid, and a window of k positions counts only if all k bytes are bases.  The
 * centre of the window that starts at s is position s + k/2 (io_utils._centre_window).  With
 * fold != 0 (k must be odd) a window whose centre base is G or T is replaced by its reverse
 * complement, so every counted k-mer has A or C in the middle.  Codes: 2 bits per letter,
 * A = 0, C = 1, G = 2, T = 3, first letter most significant (kp_kmer_parse's); the table is
 * dense, two columns of 4^k uint64 counters in the context's arena (the one kp_greedy and
 * kp_apply use: neither may be called during a session, KP_E_STATE).
 *   kp_seq_begin  k in 1..15; zeroes both columns.  KP_E_ARG: k out of range, fold with even k;
 *                 KP_E_NOMEM: the table does not fit free device memory minus 2 GiB.
 *   kp_seq_scan   one contig seq[n] (n < 2^32): every window whose centre lies in a region
 *                 [reg_begin[i], reg_end[i]) adds 1 to the background column, also where its
 *                 flanks reach outside the region; a centre whose window runs off the contig
 *                 counts nowhere.  n_regions = 0 with null pointers = the whole contig.  Regions
 *                 must be sorted, disjoint and within [0, n] (empty ones are fine), else
 *                 KP_E_ARG.  n = 0 and n < k count nothing.
 *   kp_seq_sites  the window centred at each pos[i] (0-based; pos[i] >= n is KP_E_ARG) adds 1 to
 *                 the positive column, once per occurrence; a site whose window runs off the
 *                 contig or holds an invalid byte is skipped and counted in the stats.
 *   kp_seq_end    copies out 4^k counters per column (either pointer may be NULL) and ends the
 *                 session.  Any call out of order is KP_E_STATE.
 *   kp_seq_last_stats  figures summed over the context's current or last session.
 * kp_seq_scan and kp_seq_sites copy the contig (n + 64 bytes), its work items (8 bytes per
 * 8,192 centres or region) and the site positions (8 bytes each) into a second device
 * allocation that only grows; it is not checked against the 2 GiB margin, and KP_E_NOMEM from
 * these two calls means that allocation failed (the session stays open).
 * With ctx = NULL the five calls run this thread's host session: the same per-base code
 * (classify, roll the forward and reverse-complement codes, fold) serially on the host, no
 * GPU.  kp_seq_host is one whole host session of one contig (scan != 0: the scan, of the
 * regions or of the whole contig; then the sites).  Both exist for parity and CPU tests and
 * are not a product path.
 * The scan cuts the regions into work items of at most `tile` centres, one workgroup per item
 * and step of a persistent grid.  Counters: per-workgroup uint32 LDS counters flushed with one
 * global atomic per non-zero counter for k <= 7, global 64-bit atomics into the table above
 * (the lanes of a wave that hold its first lane's code add once, together).
 * Knobs, read at each call (every setting gives the same counts): KP_SEQ_GLOBAL=1 = global
 * atomics at any k, KP_SEQ_LDS_K = largest k of the LDS path (0..7, default 7), KP_SEQ_GRID =
 * most workgroups to launch, KP_SEQ_MERGE=0 = every lane adds on its own (measurement). */
typedef struct {
    uint64_t windows;         /* windows the scans counted                                     */
    uint64_t windows_invalid; /* windows inside a contig the scans skipped for an invalid byte */
    uint64_t sites;           /* sites counted                                                 */
    uint64_t sites_skipped;   /* sites skipped (window off the contig or an invalid byte)      */
    uint64_t items;           /* work items of the scans                                       */
    double scan_ms;           /* device time of the scan kernels (HIP events; 0 on the host)   */
    uint32_t tile;            /* centres per work item at most                                 */
    uint32_t path;            /* of the last scan: 0 none or host, 1 LDS counters, 2 global
                                 atomics                                                       */
} kp_seq_stats;
int kp_seq_begin(kp_ctx *ctx, int k, int fold);
int kp_seq_scan(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end,
                uint64_t n_regions);
int kp_seq_sites(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *pos, uint64_t n_sites);
int kp_seq_end(kp_ctx *ctx, uint64_t *pos_counts, uint64_t *bg_counts);
int kp_seq_last_stats(kp_ctx *ctx, kp_seq_stats *out);
int kp_seq_host(int k, int fold, const uint8_t *seq, uint64_t n, int scan, const uint64_t *reg_begin,
                const uint64_t *reg_end, uint64_t n_regions, const uint64_t *pos, uint64_t n_sites,
                uint64_t *pos_counts, uint64_t *bg_counts, kp_seq_stats *stats);

/* Breakpoint contexts of short insertions and deletions, and background counts of both strands.
 * (No reference counterpart; the semantics are this project's own.)  Bases, validity and codes are
 * kp_seq's above; two bytes are equal if they are the same base in either case, and an invalid
 * byte equals nothing, not even itself.
 * Breakpoint b, 0 <= b <= n, is the gap before position b.  Its window at even k = 2r is
 * seq[b - r, b + r): kp_seq's window with centre b.  rc(w), the reverse complement of w, is the same
 * breakpoint read on the other strand.
 * A site is an insertion of a string I of L >= 1 bases at breakpoint b, or a deletion of
 * [s, s + L), L >= 1, s + L <= n.  Its equivalence interval [lo, hi] is the contiguous range of
 * placements that give the same mutated sequence:
 *   insertion  a = the largest j with seq[b-1-t] == I[(L-1-t) mod L] for all t < j (t < b),
 *              c = the largest j with seq[b+t] == I[t mod L] for all t < j (b + t < n);
 *              lo = b - a, hi = b + c
 *   deletion   with e = s + L: a = the largest j with seq[s-1-t] == seq[e-1-t] for all t < j
 *              (t < s), c = the largest j with seq[s+t] == seq[e+t] for all t < j (e + t < n);
 *              lo = s - a, hi = s + c
 * The chosen breakpoint p: place 0 (left, the VCF convention) = lo, 1 (right) = hi, 2 (sample) =
 * lo + (((uint64)x0 * (hi - lo + 1)) >> 32), x0 the first output word of Philox4x32-10 (the
 * generator of kp_spec_simulate) keyed by the 64-bit seed on the counter (key low word, key high
 * word, contig index, 0x494E444C); key is a uint64 the caller passes per site (kmerpapa-count: the
 * 0-based line of the site in its file), so a recurrent indel draws independently and a draw
 * depends on nothing but seed, contig and key.  The multiply-shift is not exactly uniform: the bias
 * is below 2^-32 * span.
 * An indel session has three positive columns of 4^k counters, ins, del_start and del_end, beside
 * the background column.  An insertion adds 1 to ins at code(W(p)); a deletion adds 1 to del_start
 * at code(W(p)) and 1 to del_end at code(W(p + L)).  A site any of whose windows runs off the
 * contig or holds an invalid byte is skipped whole (a deletion counts in both columns or in
 * neither) and counted in sites_skipped; it is placed first and checked after, never re-placed.
 * With both != 0 every add at (column c, code w) comes with an add at (mirror(c), rc(w)), mirror
 * swapping del_start and del_end and keeping ins, and kp_seq_scan adds 1 at code(w) and 1 at
 * code(rc(w)) for every valid window (a palindromic window: 2 in one cell).  So ins and the
 * background are rc-symmetric, del_end[w] == del_start[rc(w)], and the background sums to twice the
 * stats' windows; del_start of such a session is the table to fit deletions on ("a deletion begins
 * here, read 5' to 3'").  A site's windows, and all columns, depend only on its equivalence class
 * and on place, never on the placement the caller passed.
 *   kp_seq_begin_indel    k even, 2..14 (else KP_E_ARG); zeroes the four columns; the arena, its
 *                         exclusions and KP_E_NOMEM as kp_seq_begin_typed.  kp_seq_scan works as
 *                         in every session; kp_seq_sites and kp_seq_sites_typed are KP_E_STATE;
 *                         kp_seq_end_typed reads out and ends it ([3][4^k] ins, del_start, del_end).
 *   kp_seq_begin_strands  a plain session (k in 1..15, no folding, kp_seq_end) whose scan, with
 *                         both != 0, adds on both strands: the background of an indel fit without
 *                         the three positive columns.  kp_seq_sites in it is KP_E_STATE if both.
 *   kp_seq_indels         one contig seq[n] with index `contig`, and per site pos[i] (b or s),
 *                         del_len[i] (0 for an insertion) and key[i] (key NULL: i); insertion i is
 *                         ins[ins_off[i] .. ins_off[i + 1]) (ins_off has n_sites + 1 entries,
 *                         empty for a deletion).  resolved[n_sites][3] (may be NULL) receives lo, hi
 *                         and p, for skipped sites too.  KP_E_ARG, before anything runs, names the
 *                         first site with pos > n, a deletion past n, neither or both of
 *                         del_len and inserted bytes, or a non-base byte in the insertion; fewer
 *                         than 2^32 sites and inserted bytes per call.  KP_E_STATE outside an
 *                         indel session.  The site arrays go into the allocation kp_seq_scan uses.
 * With ctx = NULL the calls run this thread's host session, the serial definition with the same
 * per-base functions; kp_seq_indel_host is one whole host session of one contig (pos_counts
 * [3][4^k]).  On the device a wave searches one site's interval at a time, 64 positions per step
 * and side (compare, ballot, first mismatch), at most n / 64 + 1 steps; then every lane places
 * and counts its own site with global 64-bit atomics.  The both-strand scan is a separate build
 * of the scan kernel; with LDS counters (k <= 7) a launch covers at most 2^17 items per
 * workgroup, so that a uint32 counter taking 2 per centre cannot wrap (knob KP_SEQ_BOTH_STEPS,
 * 1..131072, measurement and tests: every setting gives the same counts). */
int kp_seq_begin_indel(kp_ctx *ctx, int k, int both);
int kp_seq_begin_strands(kp_ctx *ctx, int k, int both);
int kp_seq_indels(kp_ctx *ctx, const uint8_t *seq, uint64_t n, uint32_t contig, const uint64_t *pos,
                  const uint64_t *del_len, const uint64_t *key, const uint64_t *ins_off, const uint8_t *ins,
                  uint64_t n_sites, int place, uint64_t seed, uint64_t *resolved);
int kp_seq_indel_host(int k, int both, const uint8_t *seq, uint64_t n, uint32_t contig, int scan,
                      const uint64_t *reg_begin, const uint64_t *reg_end, uint64_t n_regions, const uint64_t *pos,
                      const uint64_t *del_len, const uint64_t *key, const uint64_t *ins_off, const uint8_t *ins,
                      uint64_t n_sites, int place, uint64_t seed, uint64_t *pos_counts, uint64_t *bg_counts,
                      uint64_t *resolved, kp_seq_stats *stats);

/* A fitted partition taken back to the genome: per region, how many positions fall into each
 * pattern and how many mutations the rates expect there; per position or site, which pattern.
 * (No reference counterpart.)  Bases, windows, the centre and folding are kp_seq's above; pattern
 * words are kp_apply's, and the window with code c belongs to pattern p when
 * (onehot(c) & ~patterns[p]) == 0.  All results are integers, or float64 sums in a stated order,
 * so a device session equals the host session bit for bit.
 *   kp_pred_begin    k in 1..15; the patterns are checked as kp_apply checks them and must be
 *                    pairwise disjoint (KP_E_ARG names the first pair that shares a k-mer), so a
 *                    window has at most one pattern.  Builds lut[4^k] (int32: the pattern of a
 *                    code, -1 if none) in the context's arena; KP_E_NOMEM if it does not fit free
 *                    device memory minus 2 GiB.  The session holds the arena until kp_pred_end:
 *                    kp_greedy, kp_apply, kp_seq_begin and kp_pred_begin during it are
 *                    KP_E_STATE, and so is kp_pred_begin during a kp_seq session.
 *   kp_pred_regions  one contig seq[n] (n < 2^32) and n_regions (< 2^32) half-open intervals
 *                    within [0, n], begin <= end, in any order, overlapping or not; each is one
 *                    output row and nothing is merged.  A region's centres are clipped to those
 *                    whose window lies inside the contig, [k/2, n - k + k/2 + 1).
 *                    hist[n_regions][n_patterns] (may be NULL): centres of the region whose
 *                    window is valid and belongs to the pattern.  other[n_regions][2]: [0] centres
 *                    with a valid window that matches no pattern, [1] centres whose window holds
 *                    an invalid byte or runs off the contig; a row of hist and other sums to end -
 *                    begin.  With rates[n_patterns] (may be NULL, then expected is not written)
 *                    expected[r] = acc after acc = 0.0; for p = 0 .. n_patterns - 1: acc = acc +
 *                    (double)hist[r][p] * rates[p] -- a product, then an add, in pattern order.
 *                    The n_regions x n_patterns counters live in the arena during the call:
 *                    KP_E_NOMEM if they do not fit (cut the regions into batches).
 *   kp_pred_track    pid[end - begin] (0 <= begin <= end <= n): the pattern of the window centred
 *                    at each position, -1 if none matches, -2 if the window holds an invalid byte
 *                    or runs off the contig.
 *   kp_pred_sites    the same code for the window centred at each pos[i], duplicates included;
 *                    pos[i] >= n is KP_E_ARG.
 *   kp_pred_end      ends the session.  Any call out of order is KP_E_STATE.
 *   kp_pred_last_stats  figures of the context's current or last session.
 * The contig, work items, regions and positions go into the allocation kp_seq_scan uses for them.
 * With ctx = NULL the calls run this thread's host session: the same per-base and per-code
 * functions serially, no GPU.  kp_pred_host is one whole host session of one contig: the regions
 * (if n_regions), the track of [track_begin, track_end) (if track_pid is not NULL) and the sites
 * (if n_sites).  Both exist for parity and CPU tests and are not a product path.
 * The scan cuts every clipped region into work items of at most `tile` centres, one workgroup
 * per item and step of a persistent grid; a window costs one 4-byte gather from lut.  Counters:
 * uint32 LDS counters of the workgroup that belong to one item, flushed to the region's row
 * after it with one global 64-bit atomic per non-zero counter, when n_patterns <= 16,384; else
 * global 64-bit atomics per window.  Knobs, read at each call (every setting gives the same
 * results): KP_PRED_GLOBAL=1 = global atomics at any size, KP_PRED_LDS_P = most patterns of the
 * LDS path (0..16384, default 16384), KP_PRED_GRID = most workgroups to launch. */
typedef struct {
    uint64_t assigned;  /* centres of the regions calls that fell into a pattern              */
    uint64_t unmatched; /* ... with a valid window that matches no pattern                    */
    uint64_t invalid;   /* ... with an invalid byte in the window, or a window off the contig */
    uint64_t items;     /* work items of the regions and track calls                          */
    uint64_t lut_bytes; /* size of the lookup table                                           */
    double lut_ms;      /* device time of the table's last build (HIP events; 0 on the host)  */
    double scan_ms;     /* device time of the regions and track kernels (HIP events)          */
    uint32_t tile;      /* centres per work item at most                                      */
    uint32_t path;      /* of the last regions call: 0 none or host, 1 LDS counters, 2 global
                           atomics                                                            */
} kp_pred_stats;
int kp_pred_begin(kp_ctx *ctx, int k, int fold, const uint64_t *patterns, uint32_t n_patterns, uint64_t super_word);
int kp_pred_regions(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end,
                    uint64_t n_regions, const double *rates, uint64_t *hist, uint64_t *other, double *expected);
int kp_pred_track(kp_ctx *ctx, const uint8_t *seq, uint64_t n, uint64_t begin, uint64_t end, int32_t *pid);
int kp_pred_sites(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *pos, uint64_t n_sites, int32_t *pid);
int kp_pred_end(kp_ctx *ctx);
int kp_pred_last_stats(kp_ctx *ctx, kp_pred_stats *out);
int kp_pred_host(int k, int fold, const uint64_t *patterns, uint32_t n_patterns, uint64_t super_word,
                 const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end, uint64_t n_regions,
                 const double *rates, uint64_t *hist, uint64_t *other, double *expected, uint64_t track_begin,
                 uint64_t track_end, int32_t *track_pid, const uint64_t *pos, uint64_t n_sites, int32_t *site_pid,
                 kp_pred_stats *stats);

/* The whole mutation spectrum in one genome pass: counting, and a fitted partition per mutation
 * type taken back to the genome together.  (No reference counterpart.)  Bases, windows, the centre
 * and folding are kp_seq's above, pattern words and matching kp_apply's.
 * Types and slots.  A window's centre base is the REF of every mutation at its centre -- after
 * folding, if the window was replaced by its reverse complement, and then ALT is complemented too.
 * The slot of an ALT is its rank (0..2) among the bases other than REF in ACGT order, and the type
 * id is t = 3 * code(REF) + slot: 0..11 = A>C A>G A>T C>A C>G C>T G>A G>C G>T T>A T>C T>G; with
 * folding only 0..5 occur.
 * Typed counting (a kp_seq session with three positive columns, one per slot):
 *   kp_seq_begin_typed  as kp_seq_begin; four columns of 4^k uint64 (32 GiB at k = 15) against the
 *                       same "free minus 2 GiB" rule.
 *   kp_seq_sites_typed  alt[i] = the ALT base of site i on the forward strand, one of ACGTacgt (any
 *                       other byte is KP_E_ARG, checked on the host before anything is launched).  The
 *                       window is classified, rolled and folded as kp_seq_sites does; the site adds 1
 *                       to column slot(centre base, ALT) at the window's code.  A site whose window
 *                       runs off the contig or holds an invalid byte, or whose ALT equals the centre
 *                       base, is skipped and counted in sites_skipped.
 *   kp_seq_end_typed    pos_counts[3][4^k], bg_counts[4^k] (either may be NULL); ends the session.
 * kp_seq_scan and kp_seq_last_stats work in both kinds of session; kp_seq_sites / kp_seq_end in a
 * typed session and kp_seq_sites_typed / kp_seq_end_typed in a plain one are KP_E_STATE.
 * Spectrum sessions:
 *   kp_spec_begin    k in 1..15 (fold needs an odd k); patterns[n_patterns] of every type in one
 *                    list, ptype[p] in 0..11 (0..5 with fold) the type of pattern p; a type may have
 *                    no pattern.  KP_E_ARG, naming the first offender: a pattern with an empty
 *                    position or bits above position k, a type out of range, a pattern whose centre
 *                    position (k/2) does not allow exactly the REF base of its type, two patterns
 *                    of one type that share a k-mer, n_patterns = 0.  (Patterns of different types
 *                    with the same slot differ in the centre, so a code has at most one pattern per
 *                    slot.)  Builds lut[4^k] of 16-byte entries {pattern of slot 0, 1, 2, -1}, ids
 *                    indexing `patterns`, -1 = none, in the context's arena; KP_E_NOMEM if it does
 *                    not fit free device memory minus 2 GiB (16 GiB at k = 15).  The session holds
 *                    the arena until kp_spec_end: kp_greedy, kp_apply, kp_seq_begin*, kp_pred_begin
 *                    and kp_spec_begin during it are KP_E_STATE, and so is kp_spec_begin during a
 *                    kp_seq or kp_pred session.  These exclusions hold for a device context
 *                    only: the host sessions (ctx = NULL) of kp_seq, kp_pred and kp_spec share no
 *                    arena and are independent of each other.
 *   kp_spec_regions  regions as kp_pred_regions'.  hist[n_regions][n_patterns] (may be NULL).
 *                    other[n_regions][4]: [s], s = 0..2, centres with a valid window and no pattern
 *                    in slot s; [3] centres whose window holds an invalid byte or runs off the
 *                    contig.  For every region and slot s the hist entries of the patterns with
 *                    ptype % 3 == s, other[s] and other[3] sum to end - begin.  With
 *                    rates[n_patterns] (may be NULL, then expected is not written)
 *                    expected[r][t], t = 0..11, = acc after acc = 0.0; for p ascending with
 *                    ptype[p] == t: acc = acc + (double)hist[r][p] * rates[p] -- a product, then an
 *                    add; 0.0 for a type without patterns.
 *   kp_spec_track    pid[3][end - begin], slot-major: per slot the values of kp_pred_track.
 *   kp_spec_sites    pid[i] = the pattern in the slot of the (folded) ALT of site i, -1 if none, -2
 *                    if the window holds an invalid byte or runs off the contig, -3 if ALT equals
 *                    the centre base; alt and pos as kp_seq_sites_typed's.
 *   kp_spec_end, kp_spec_last_stats  as kp_pred's; in the stats a centre counts once per slot:
 *                    assigned + unmatched = 3 x the centres with a valid window.
 * With ctx = NULL the calls run this thread's host session, serially with the same per-base and
 * per-code functions; kp_spec_host is one whole host session of one contig, as kp_pred_host.
 * The scan is kp_pred's with one 16-byte gather and up to three counter adds per valid window:
 * uint32 LDS counters per item when n_patterns <= 16,384, global 64-bit atomics otherwise.  Knobs,
 * read at each call (every setting gives the same results): KP_SPEC_GLOBAL, KP_SPEC_LDS_P and
 * KP_SPEC_GRID, with the meaning of their KP_PRED_* counterparts.
 * Simulation (a call of a spectrum session): a random mutation set drawn from the model.
 *   kp_spec_simulate  Per position of the regions: the window, its validity, centre and folding
 *                    are kp_spec_regions'; an invalid window, or one that runs off the contig, draws
 *                    nothing.  A valid window with code c reads lut[c] = {id0, id1, id2, -1};
 *                    r_s = id_s >= 0 ? rates[id_s] * scale : 0.0 (a product); c0 = r0, c1 = c0 + r1,
 *                    c2 = c1 + r2 (adds in that order, no contraction).  With the uniform number u
 *                    below the position mutates into slot 0 if u < c0, else slot 1 if u < c1, else
 *                    slot 2 if u < c2, else not at all: at most one mutation per position, each
 *                    type's marginal probability exactly its rate.  (Where c2 == 0.0 the generator
 *                    may be skipped: the result is the same.)  The slots are those of the counted
 *                    (folded) strand; the reported ALT is on the forward strand -- if the window
 *                    was replaced by its reverse complement the slot's base is complemented back --
 *                    as upper-case ASCII.
 *                    u: Philox4x32 with 10 rounds, key (seed low 32 bits, seed high 32 bits),
 *                    counter (position low 32, position high 32, contig_id, replicate), position =
 *                    the 0-based position in the contig.  One round on counter (c0, c1, c2, c3) and
 *                    key (k0, k1): p0 = 0xD2511F53 * c0 and p1 = 0xCD9E8D57 * c2 as 64-bit products;
 *                    the new counter is (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)); then
 *                    k0 += 0x9E3779B9, k1 += 0xBB67AE85 mod 2^32.  With the output x0..x3,
 *                    u = (double)(((uint64)x1 << 32 | x0) >> 11) * 2^-53, both steps exact.  (The
 *                    published Random123 known answers hold: the all-zero counter and key give
 *                    6627e8d5 e169c58d bc57ac4c 9b00dbd8.)  The draw depends on (seed, contig_id,
 *                    position, replicate) and the model only -- not on the regions asked for, the
 *                    grid, knobs or arrival order -- and the device result equals the host result
 *                    bit for bit.
 *                    Regions are clipped as kp_spec_regions clips them and must be ascending and
 *                    disjoint (reg_begin[i] >= reg_end[i - 1], begin <= end; empty and adjacent
 *                    regions are fine).  *n_hits is always the total number of hits.  out_pos,
 *                    out_alt and out_pid (the pattern whose rate produced the hit) receive the hits
 *                    in ascending position order only if *n_hits <= cap; otherwise they are left
 *                    untouched and the call still returns KP_OK: the caller repeats it with a
 *                    larger cap, and the repeat is exact by construction.  KP_E_STATE outside a
 *                    session.  KP_E_ARG, checked on the host before any launch and naming the first
 *                    offender: a rate or scale that is not finite or is negative; a REF base for
 *                    which the sum over its three types of the type's largest rates[p] * scale
 *                    exceeds 1.0; unsorted or overlapping regions.
 *   kp_spec_last_sim  figures of the session's last kp_spec_simulate call.
 * With ctx = NULL the draw runs serially in the host session with the same functions.  On the
 * device it is an ordered two-pass compaction: a count kernel (the scan's roll and gathers, the
 * draw, one plain store of the item's hits), an exclusive scan of the items' hits whose total is
 * read back (the call ends there if it exceeds cap), and a write kernel that draws again and puts
 * each hit at item offset + thread offset + rank; the order never depends on atomics.  Knob, read at
 * each call (every setting gives the same results): KP_SIM_GRID caps the grid.
 * Null tables (a call of a spectrum session): many replicates of that draw, counted per region.
 *   kp_spec_null     Regions are kp_spec_regions' regions: in any order, overlapping or not, empty
 *                    or not, clipped the same way, nothing merged.  Without by_type the output is
 *                    counts[n_regions][n_reps]: counts[r][j] = the number of positions p with
 *                    reg_begin[r] <= p < reg_end[r] at which kp_spec_simulate with the same (seq,
 *                    contig_id, rates, scale, seed) and replicate = rep_first + j draws a hit -- the
 *                    window, its validity, the table entry, c0 <= c1 <= c2, u and the slot exactly as
 *                    described there.  With by_type the output is counts[n_regions][n_reps][12],
 *                    indexed by the type id ptype[pid] of the pattern that produced the hit; ids
 *                    6..11 stay 0 under folding, and the 12 entries sum to the entry without
 *                    by_type.  The result depends on (seed, contig_id, position, replicate) and the
 *                    model only -- not on the other regions, on how replicates are batched, on the
 *                    grid, knobs or arrival order: a call with (rep_first = a, n_reps = b) equals
 *                    columns a .. a + b - 1 of a call with (rep_first = 0, n_reps = a + b).  Counts
 *                    are integers, so the device result equals the host result bit for bit; a count
 *                    is at most the region's length, below 2^32 as a contig is, so uint32 cannot wrap.
 *                    KP_E_STATE outside a session.  KP_E_ARG, checked on the host before any launch
 *                    and naming the first offender (counts is left untouched): counts or rates NULL;
 *                    n_reps = 0; rep_first + n_reps > 2^32; a rate or scale kp_spec_simulate
 *                    rejects; a region with begin > end or past the contig.  KP_E_NOMEM if the table
 *                    does not fit the arena beside the lookup table (free device memory minus 2 GiB);
 *                    the lookup table stays where it was, or is built again if the arena grew.
 *   kp_spec_last_null  figures of the session's last kp_spec_null call.
 * With ctx = NULL the call runs serially in the host session with the same functions.  The
 * comparison u < c is made on integers: u = m * 2^-53 with m the 53 bits of the generator's output,
 * and m < ceil(c * 2^53) holds exactly when u < c does (the product is exact for c in [0, 1]).  On
 * the device one kernel runs a persistent grid over (work item, replicate chunk) pairs: per batch of
 * the roll the threads stage every window's three thresholds in LDS, then each wave walks staged
 * windows with consecutive replicates on its lanes -- the first Philox round does not depend on the
 * replicate and is done once per window -- and a hit adds to the item's uint32 LDS counter
 * [replicate][type]; after the item each non-zero counter goes to counts with one global atomic.  A
 * chunk holds at most 3,072 replicates (256 with by_type); more replicates take several passes over
 * the item.  Knobs, read at each call (every setting gives the same table): KP_NULL_REPS caps the
 * replicates per pass, KP_NULL_GRID the grid.
 * Coding consequences (calls of a spectrum session): expected mutations per transcript by class.
 *   Transcripts.     A transcript t has a strand tx_strand[t] (0 = +, 1 = -) and the CDS segments
 *                    tx_first[t] .. tx_first[t + 1] - 1 of seg_begin / seg_end on the call's contig:
 *                    0-based half-open, non-empty, ascending and non-overlapping (abutting segments
 *                    have no intron between them); tx_first[0] = 0, tx_first[n_tx] = n_segs.  The
 *                    lengths of a transcript's segments sum to a multiple of 3.  Transcripts may
 *                    overlap each other in any way; each is computed on its own.  KP_E_ARG, checked on
 *                    the host before any launch and naming the first offending transcript, for
 *                    anything else; also splice > 8.
 *   Codons.          The spliced index of position g of segment e is j = (the lengths of the
 *                    transcript's segments before e) + g - seg_begin[e], in genomic orientation on
 *                    both strands.  The codon of g is the spliced bytes x0 x1 x2 at 3 (j / 3) .. + 2
 *                    -- it may span two or three segments -- read on the - strand as (comp x2, comp
 *                    x1, comp x0).  Lower case counts as upper case.
 *   Classes.         Every coding position has three (position, forward ALT) pairs, the bases other
 *                    than its own.  A pair's class comes from the standard genetic code applied to
 *                    the transcript-strand codon before and after the change: 0 synonymous (the same
 *                    amino acid, or stop to stop), 1 missense, 2 nonsense (amino acid to stop), 3
 *                    stop-lost (stop to amino acid); 4 = every pair of an essential splice position:
 *                    an intronic base within `splice` bases of either end of an intron between two
 *                    consecutive segments -- for the intron [a, b) the positions [a, min(a + splice,
 *                    b)) and [max(b - splice, a), b), each once.  A coding position whose codon holds
 *                    a byte that is none of ACGTacgt, and a splice position whose own byte is none,
 *                    has no class and counts once in other[7].
 *   Rates.           The pattern of a pair is kp_spec_sites' (the window's code, the slot of the
 *                    folded ALT).  The class never depends on the window: a pair whose window is
 *                    invalid or leaves the contig still has a class and is counted, without a pattern.
 *   kp_spec_coding   hist[n_tx][5][n_patterns] (may be NULL): the pairs of class c whose pattern is
 *                    p.  other[n_tx][8]: [0..4] all pairs per class, rated or not (the mutational
 *                    opportunity); [5] pairs with an invalid window; [6] pairs with a valid window
 *                    and no pattern in their slot; [7] positions without a class.  So sum(other[0..4])
 *                    = sum(hist) + other[5] + other[6], and 3 x positions = sum(other[0..4]) + 3 x
 *                    other[7].  With rates (may be NULL) expected[n_tx][5][12]: kp_spec_regions' sum
 *                    of row [t][c] of hist per type id.  Other argument and state errors, and the
 *                    arena, as kp_spec_regions'.
 *   kp_spec_coding_sites  One result per (site, transcript) pair i: position pos[i] with the forward
 *                    ALT alt[i] (checked as kp_spec_sites checks them) in transcript tx[i] < n_tx.
 *                    cls[i] = the class 0..4, or -1: the position is neither coding nor an essential
 *                    splice position of that transcript; -2: it has no class; -3: ALT equals REF (in
 *                    this order of precedence).  pid[i] as kp_spec_sites' output.  codons[i] = the
 *                    transcript-strand REF codon (16 b0 + 4 b1 + b2, ACGT digits) | ALT codon << 6
 *                    for classes 0..3, else 0.
 *   kp_spec_last_coding  figures of the session's last kp_spec_coding call.
 * With ctx = NULL the calls run serially in the host session with the same per-pair functions.  On
 * the device kp_spec_coding runs kp_spec_regions' persistent grid and roll over pieces of one segment
 * or of one splice interval; a record per segment carries the transcript, the strand, the spliced
 * index of its first base and the two spliced bases before and after it, so nothing outside the
 * segment is read for a codon.  Counters [5][n_patterns] are uint32 in LDS per item while n_patterns
 * <= 3,276 (5 x 4 x n_patterns <= 64 KiB), global 64-bit atomics otherwise.  Knobs, read at each call
 * (every setting gives the same results): KP_CODING_GLOBAL, KP_CODING_LDS_P and KP_CODING_GRID, with
 * the meaning of their KP_SPEC_* counterparts.
 * Null tables per transcript and class (a call of a spectrum session): kp_spec_null's replicates,
 * binned as kp_spec_coding bins.
 *   kp_spec_coding_null  Transcripts, codons, classes and `splice` exactly as kp_spec_coding defines
 *                    them; rates, scale, seed, contig_id, rep_first and n_reps exactly as
 *                    kp_spec_null's.  counts[n_tx][n_reps][5]: counts[t][j][c] = the number of
 *                    positions p that are a coding or essential splice position of transcript t and
 *                    at which kp_spec_simulate with the same (seq, contig_id, rates, scale, seed) and
 *                    replicate = rep_first + j draws a hit whose forward ALT a gives class c in
 *                    kp_spec_coding_sites (p, a, t).  A hit at a position without a class (cls = -2)
 *                    enters no column and is counted in the stats as `unclassed`.  A position whose
 *                    window is invalid or leaves the contig draws nothing, so unlike kp_spec_coding
 *                    no clipped centre is made up for on the host.  The result depends on (seed,
 *                    contig_id, position, replicate), the model and transcript t only -- not on the
 *                    other transcripts, on how replicates are batched, on the grid, knobs or arrival
 *                    order: (rep_first = a, n_reps = b) equals columns a .. a + b - 1 of (0, a + b).
 *                    Counts are integers, so the device result equals the host result bit for bit; a
 *                    count is at most the transcript's positions, below 2^32, so uint32 cannot wrap.
 *                    KP_E_STATE outside a session.  KP_E_ARG, checked on the host before any launch
 *                    (counts is left untouched): whatever kp_spec_coding rejects about the transcript
 *                    table and splice, and whatever kp_spec_null rejects about counts, rates, scale,
 *                    n_reps and rep_first.  KP_E_NOMEM if the table and the staged records (32 bytes
 *                    per position) do not fit the arena beside the lookup table, which stays where it
 *                    was or is built again if the arena grew, as in kp_spec_null.
 *   kp_spec_last_coding_null  figures of the session's last kp_spec_coding_null call; all but the
 *                    times, passes and reps_per_pass are equal between the host and a device session.
 * With ctx = NULL the call runs serially in the host session with the same per-pair functions.  On
 * the device the work that does not depend on the replicate runs once: a stage kernel with one
 * thread per (transcript, position) finds its segment or splice interval by a bounded binary search
 * over host-computed dense offsets, reads its window, table entry and rates, and stores a 32-byte
 * record -- the three integer thresholds of kp_spec_null (T2 = 0: draws nothing), the position and
 * the class of each ALT slot -- at item base + index, so a transcript's records are contiguous and
 * nothing is compacted.  A draw kernel then runs a persistent grid over (piece of at most 4,095
 * records of one transcript, replicate chunk) units: records are wave-uniform, lanes hold
 * consecutive replicates, the first Philox round runs once per record and the other nine once per
 * lane, the five class counters of a lane are 12-bit fields of one 64-bit register, and each
 * non-zero (transcript, replicate, class) leaves with one global atomic.  A chunk holds at most 256
 * replicates, one per thread; with 128 or fewer the four waves split a piece's records.  More
 * replicates take several passes over the records, never over the sequence.  Knobs, read at each
 * call (every setting gives the same table): KP_CNULL_REPS caps the replicates per pass,
 * KP_CNULL_GRID both grids. */
typedef struct {
    uint64_t windows; /* valid windows inside the regions                                          */
    uint64_t hits;    /* mutations drawn                                                           */
    uint64_t items;   /* work items                                                                */
    double count_ms;  /* device time of the count and offsets kernels (HIP events; 0 on the host)  */
    double write_ms;  /* device time of the write kernel (HIP events; 0 on the host or if not run) */
} kp_spec_sim_stats;
typedef struct {
    uint64_t windows;       /* valid windows, summed over the regions                                */
    uint64_t draws;         /* windows with c2 > 0, times n_reps                                     */
    uint64_t hits;          /* the sum of the table                                                  */
    uint64_t items;         /* work items                                                            */
    uint32_t passes;        /* replicate chunks each item was run in (1 on the host)                 */
    uint32_t reps_per_pass; /* replicates per chunk, the last one may hold fewer (n_reps on the host) */
    double null_ms;         /* device time of the kernel (HIP events; 0 on the host)                 */
} kp_spec_null_stats;
typedef struct {
    uint64_t assigned;  /* (centre, slot) pairs of the regions calls that fell into a pattern      */
    uint64_t unmatched; /* ... with a valid window and no pattern in the slot                      */
    uint64_t invalid;   /* centres with an invalid byte in the window, or a window off the contig  */
    uint64_t items;     /* work items of the regions and track calls                               */
    uint64_t lut_bytes; /* size of the lookup table                                                */
    double lut_ms;      /* device time of the table's last build (HIP events; 0 on the host)       */
    double scan_ms;     /* device time of the regions and track kernels (HIP events)               */
    uint32_t tile;      /* centres per work item at most                                           */
    uint32_t path;      /* of the last regions call: 0 none or host, 1 LDS counters, 2 global
                           atomics                                                                 */
} kp_spec_stats;
typedef struct {
    uint64_t items;     /* work items                                                              */
    uint64_t positions; /* coding and essential splice positions, summed over the transcripts      */
    uint64_t pairs;     /* (position, ALT) pairs with a class: the sum of other[0..4]              */
    double scan_ms;     /* device time of the scan kernel (HIP events; 0 on the host)              */
    uint32_t path;      /* 0 none or host, 1 LDS counters, 2 global atomics                        */
} kp_spec_coding_stats;
typedef struct {
    uint64_t positions;     /* coding and essential splice positions, summed over the transcripts    */
    uint64_t drawing;       /* ... among them with a valid window and c2 > 0                         */
    uint64_t hits;          /* the sum of the table                                                  */
    uint64_t unclassed;     /* hits at positions without a class, summed over the replicates         */
    uint32_t passes;        /* replicate chunks the records were drawn in (1 on the host)            */
    uint32_t reps_per_pass; /* replicates per chunk, the last one may hold fewer (n_reps on the host) */
    double stage_ms;        /* device time of the stage kernel (HIP events; 0 on the host)           */
    double draw_ms;         /* device time of the draw kernel (HIP events; 0 on the host)            */
} kp_spec_coding_null_stats;
int kp_seq_begin_typed(kp_ctx *ctx, int k, int fold);
int kp_seq_sites_typed(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *pos, const uint8_t *alt,
                       uint64_t n_sites);
int kp_seq_end_typed(kp_ctx *ctx, uint64_t *pos_counts, uint64_t *bg_counts);
int kp_spec_begin(kp_ctx *ctx, int k, int fold, const uint64_t *patterns, const uint32_t *ptype, uint32_t n_patterns);
int kp_spec_regions(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end,
                    uint64_t n_regions, const double *rates, uint64_t *hist, uint64_t *other, double *expected);
int kp_spec_track(kp_ctx *ctx, const uint8_t *seq, uint64_t n, uint64_t begin, uint64_t end, int32_t *pid);
int kp_spec_sites(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *pos, const uint8_t *alt, uint64_t n_sites,
                  int32_t *pid);
int kp_spec_end(kp_ctx *ctx);
int kp_spec_last_stats(kp_ctx *ctx, kp_spec_stats *out);
int kp_spec_host(int k, int fold, const uint64_t *patterns, const uint32_t *ptype, uint32_t n_patterns, const uint8_t *seq,
                 uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end, uint64_t n_regions, const double *rates,
                 uint64_t *hist, uint64_t *other, double *expected, uint64_t track_begin, uint64_t track_end,
                 int32_t *track_pid, const uint64_t *pos, const uint8_t *alt, uint64_t n_sites, int32_t *site_pid,
                 kp_spec_stats *stats);
int kp_spec_simulate(kp_ctx *ctx, const uint8_t *seq, uint64_t n, uint32_t contig_id, const uint64_t *reg_begin,
                     const uint64_t *reg_end, uint64_t n_regions, const double *rates, double scale, uint64_t seed,
                     uint32_t replicate, uint64_t cap, uint64_t *out_pos, uint8_t *out_alt, int32_t *out_pid,
                     uint64_t *n_hits);
int kp_spec_last_sim(kp_ctx *ctx, kp_spec_sim_stats *out);
int kp_spec_null(kp_ctx *ctx, const uint8_t *seq, uint64_t n, uint32_t contig_id, const uint64_t *reg_begin,
                 const uint64_t *reg_end, uint64_t n_regions, const double *rates, double scale, uint64_t seed,
                 uint32_t rep_first, uint32_t n_reps, int by_type, uint32_t *counts);
int kp_spec_last_null(kp_ctx *ctx, kp_spec_null_stats *out);
int kp_spec_coding(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *seg_begin, const uint64_t *seg_end,
                   uint64_t n_segs, const uint64_t *tx_first, const uint8_t *tx_strand, uint64_t n_tx, uint32_t splice,
                   const double *rates, uint64_t *hist, uint64_t *other, double *expected);
int kp_spec_coding_sites(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *seg_begin, const uint64_t *seg_end,
                         uint64_t n_segs, const uint64_t *tx_first, const uint8_t *tx_strand, uint64_t n_tx,
                         uint32_t splice, const uint64_t *pos, const uint8_t *alt, const uint32_t *tx, uint64_t n_pairs,
                         int32_t *cls, int32_t *pid, uint32_t *codons);
int kp_spec_last_coding(kp_ctx *ctx, kp_spec_coding_stats *out);
int kp_spec_coding_null(kp_ctx *ctx, const uint8_t *seq, uint64_t n, uint32_t contig_id, const uint64_t *seg_begin,
                        const uint64_t *seg_end, uint64_t n_segs, const uint64_t *tx_first, const uint8_t *tx_strand,
                        uint64_t n_tx, uint32_t splice, const double *rates, double scale, uint64_t seed, uint32_t rep_first,
                        uint32_t n_reps, uint32_t *counts);
int kp_spec_last_coding_null(kp_ctx *ctx, kp_spec_coding_null_stats *out);

/* An indel model taken back to the genome on both strands: an insertion and a deletion partition,
 * fitted on the ins and del_start columns of a both-strand indel session, applied per breakpoint.
 * (No reference counterpart.)  Bases, windows, validity and codes are kp_seq's above, pattern words
 * and matching kp_apply's; breakpoints and windows are those of the indel counting block: the
 * window of breakpoint b at k = 2r is W(b) = seq[b - r, b + r).
 * Strands.  del_start of a both-strand session means "a deletion begins here, read 5' to 3'": on the
 * forward strand the rate of a deletion starting at b is r(W(b)), and r(rc(W(b))) is the rate of one
 * ending at b.  A fitted partition is not rc-symmetric even where its table is (the lattice does not
 * force P and rc(P) into one partition), so an insertion rate needs both look-ups as well.  Strand
 * 0 of a result is the look-up of W(b), strand 1 that of rc(W(b)).
 *   kp_ispec_begin   k even, 2..14; patterns[n_patterns] of both kinds in one list, pkind[p] = 0
 *                    (ins) or 1 (del); a kind may have no pattern.  KP_E_ARG, naming the first
 *                    offender: a pattern with an empty position or bits above position k, a kind out
 *                    of range, two patterns of one kind that share a k-mer (across kinds is fine),
 *                    n_patterns = 0.  Builds lut[4^k] of 16-byte entries {ins pattern of c, ins
 *                    pattern of rc(c), del pattern of c, del pattern of rc(c)}, ids indexing
 *                    `patterns`, -1 = none, in the context's arena (4 GiB at k = 14): the reverse
 *                    complement is resolved when the table is built, so the scan pays one 16-byte
 *                    gather per breakpoint and needs only the forward code.  The arena rules, the
 *                    exclusions (kp_greedy, kp_apply, kp_seq_begin*, kp_pred_begin, kp_spec_begin and
 *                    kp_ispec_begin during it are KP_E_STATE, and so is kp_ispec_begin during a
 *                    kp_seq, kp_pred or kp_spec session; device contexts only) and KP_E_NOMEM are
 *                    kp_spec_begin's.
 *   kp_ispec_regions regions and clipping as kp_pred_regions': any order, overlapping or not, each
 *                    one output row; a region's breakpoints are begin <= b < end.
 *                    hist[n_regions][2][n_patterns] (may be NULL): strand 0 counts the breakpoints
 *                    whose window matches the pattern, strand 1 those whose window's reverse
 *                    complement matches it.  other[n_regions][5]: [2 * kind + strand] valid windows
 *                    with no pattern of that kind on that strand, [4] windows that hold an invalid
 *                    byte or run off the contig.  For every region, kind and strand the hist entries
 *                    of that kind, other[2 * kind + strand] and other[4] sum to end - begin.  With
 *                    rates[n_patterns] (may be NULL, then expected is not written)
 *                    expected[n_regions][4] = ins forward, ins rc, del start (strand 0), del end
 *                    (strand 1), each acc after acc = 0.0; for p ascending of that kind: acc = acc +
 *                    (double)hist[r][strand][p] * rates[p].  The counters live in the arena during
 *                    the call: KP_E_NOMEM if they do not fit.
 *   kp_ispec_track   pid[4][end - begin], plane-major in the order of the table entry; values as
 *                    kp_pred_track's: id, -1 for none, -2 for an invalid window.
 *   kp_ispec_sites   site arrays, argument checks, equivalence interval, placement and its Philox
 *                    draw are exactly kp_seq_indels'.  resolved[n_sites][3] (may be NULL) = lo, hi, p,
 *                    identical to what a counting session returns for the same (place, seed, contig,
 *                    key).  pid[n_sites][2]: for an insertion the ins pattern of W(p) and of rc(W(p));
 *                    for a deletion the del pattern of W(p), its start, and of rc(W(p + L)), its end
 *                    read on the other strand; -1 where no pattern matches; both -2 where the
 *                    counting would skip the site whole (placed first, checked after, never
 *                    re-placed).
 *   kp_ispec_end, kp_ispec_last_stats  as kp_spec's; in the stats a breakpoint counts once per kind
 *                    and strand: assigned + unmatched = 4 x the breakpoints with a valid window.
 * Any call out of order is KP_E_STATE.  With ctx = NULL the calls run this thread's host session,
 * serially with the same per-base and per-code functions; kp_ispec_host is one whole host session of
 * one contig, as kp_spec_host (the sites with contig index `contig`).
 * The scan is kp_spec's with fold = 0, one 16-byte gather and up to four counter adds per valid
 * window: 2 x n_patterns uint32 LDS counters per item (strand-major) when n_patterns <= 8,192 -- the
 * spectrum scan's 64 KiB -- and global 64-bit atomics otherwise.  The sites kernel runs
 * kp_seq_indels' wave-cooperative interval search, then two table look-ups per site and no atomics
 * on tables.  Knobs, read at each call (every setting gives the same results): KP_ISPEC_GLOBAL,
 * KP_ISPEC_LDS_P (0..8192) and KP_ISPEC_GRID, with the meaning of their KP_SPEC_* counterparts. */
typedef struct {
    uint64_t assigned;      /* (breakpoint, kind, strand) triples of the regions calls with a pattern   */
    uint64_t unmatched;     /* ... with a valid window and no pattern of the kind on the strand         */
    uint64_t invalid;       /* breakpoints with an invalid byte in the window, or a window off the contig */
    uint64_t items;         /* work items of the regions and track calls                                */
    uint64_t lut_bytes;     /* size of the lookup table                                                 */
    double lut_ms;          /* device time of the table's last build (HIP events; 0 on the host)        */
    double scan_ms;         /* device time of the regions and track kernels (HIP events)                */
    uint32_t tile;          /* breakpoints per work item at most                                        */
    uint32_t path;          /* of the last regions call: 0 none or host, 1 LDS counters, 2 global atomics */
    uint64_t sites;         /* sites of the sites calls that got their patterns                         */
    uint64_t sites_skipped; /* ... skipped whole (both ids -2)                                          */
    double sites_ms;        /* device time of the sites kernel (HIP events; 0 on the host)              */
} kp_ispec_stats;
int kp_ispec_begin(kp_ctx *ctx, int k, const uint64_t *patterns, const uint32_t *pkind, uint32_t n_patterns);
int kp_ispec_regions(kp_ctx *ctx, const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end,
                     uint64_t n_regions, const double *rates, uint64_t *hist, uint64_t *other, double *expected);
int kp_ispec_track(kp_ctx *ctx, const uint8_t *seq, uint64_t n, uint64_t begin, uint64_t end, int32_t *pid);
int kp_ispec_sites(kp_ctx *ctx, const uint8_t *seq, uint64_t n, uint32_t contig, const uint64_t *pos,
                   const uint64_t *del_len, const uint64_t *key, const uint64_t *ins_off, const uint8_t *ins,
                   uint64_t n_sites, int place, uint64_t seed, uint64_t *resolved, int32_t *pid);
int kp_ispec_end(kp_ctx *ctx);
int kp_ispec_last_stats(kp_ctx *ctx, kp_ispec_stats *out);
int kp_ispec_host(int k, const uint64_t *patterns, const uint32_t *pkind, uint32_t n_patterns, const uint8_t *seq, uint64_t n,
                  uint32_t contig, const uint64_t *reg_begin, const uint64_t *reg_end, uint64_t n_regions,
                  const double *rates, uint64_t *hist, uint64_t *other, double *expected, uint64_t track_begin,
                  uint64_t track_end, int32_t *track_pid, const uint64_t *pos, const uint64_t *del_len, const uint64_t *key,
                  const uint64_t *ins_off, const uint8_t *ins, uint64_t n_sites, int place, uint64_t seed,
                  uint64_t *resolved, int32_t *site_pid, kp_ispec_stats *stats);

/* Host-only (no GPU needed): the cross-validation fold split of CV_tools.py
 * make_all_folds_contextD_patterns :44-57 / sample :5-27 with numpy's legacy
 * RandomState stream.  mt_key[624] / *mt_pos = the MT19937 state of the caller's
 * RandomState (RandomState.get_state()[1:3]), advanced in place exactly as numpy would.
 * colors[n] = ball counts per colour; folds[n][nf] receives each colour's fold counts
 * (folds 0..nf-2 sampled, the last takes the remainder). */
int kp_fold_split(uint32_t *mt_key, int32_t *mt_pos, const uint64_t *colors, uint64_t n, int nf, uint64_t *folds);
/* One fold of that split: CV_tools.py sample :5-27 (m balls drawn colour by colour from
 * colors[n]; out[n] = the balls drawn of each colour), same RNG state convention. */
int kp_fold_sample(uint32_t *mt_key, int32_t *mt_pos, const uint64_t *colors, uint64_t n, uint64_t m,
                   uint64_t *out);

/* k-mer count text (host code, no GPU).  Parses `nbytes` of file text into a table of
 * unique k-mers as 2-bit codes (A=0 C=1 G=2 T=3, first letter most significant: code
 * order = sorted k-mer order) with counts:
 *   columns = 2: "kmer count" lines (io_utils.read_dict :82-136).  Counts of equal k-mers
 *     are summed into c0 (c1 = 0); total0 = sum of kept counts.  length > 0 keeps the
 *     central `length` letters (width//2 - length//2 ...); with a super pattern and
 *     length <= 0 the pattern's length is used.  Negative counts are an error.
 *   columns = 3: "kmer positive background" lines (read_joint_kmer_counts :3-46).  The
 *     last line of a k-mer wins: c0 = positive, c1 = background - positive (an error if
 *     negative); total0 = n_negative_total, total1 = n_positive_total over every kept line.
 * super_pattern (IUPAC, may be NULL or "") keeps only matching k-mers.  Lines whose k-mer
 * has a letter other than A/C/G/T are skipped; a line with the wrong number of tokens,
 * a bad count or k-mers of different lengths is KP_E_ARG with kp_last_error() text. */
typedef struct kp_kmer_table kp_kmer_table;
int kp_kmer_parse(const char *text, uint64_t nbytes, int columns, const char *super_pattern, int length,
                  kp_kmer_table **out);
int kp_kmer_table_info(const kp_kmer_table *t, uint64_t *n, int32_t *k, int64_t *total0, int64_t *total1);
/* codes[n], c0[n], c1[n]: caller-allocated (n from kp_kmer_table_info) */
int kp_kmer_table_copy(const kp_kmer_table *t, uint64_t *codes, int64_t *c0, int64_t *c1);
void kp_kmer_table_free(kp_kmer_table *t);

/* The long output table (host code, no GPU): cli.py:301-316 with -l prints, for every k-mer
 * of every pattern, f"{context} {c_neg} {c_pos} {c_rate}" + the pattern's tail
 * " {pattern} {p_neg} {p_pos} {p_rate}\n", c_rate = c_pos / (c_pos + c_neg) as Python's
 * repr() writes a float.  kmers: n * k letters; pid[i] = row i's tail; tail t is
 * tails[tail_off[t] .. tail_off[t + 1]).  Writes at most cap bytes to out, *out_len = bytes
 * written.  KP_E_ARG if cap is too small or a row has c_pos + c_neg == 0 (where Python
 * raises ZeroDivisionError). */
int kp_format_long_rows(const char *kmers, int k, const int64_t *c_neg, const int64_t *c_pos, const uint32_t *pid,
                        uint64_t n, const char *tails, const uint64_t *tail_off, uint64_t n_tails, char *out,
                        uint64_t cap, uint64_t *out_len);
/* Python repr() of x[0..n), one per line (the float format of kp_format_long_rows). */
int kp_py_repr(const double *x, uint64_t n, char *out, uint64_t cap, uint64_t *out_len);

#ifdef __cplusplus
}
#endif
#endif
