// kp_hip.hip -- gfx950 kernels and C-ABI of the blocked lattice DP (libkmerpapa_hip.so).
//
// The sweep is VALUE-ONLY (kp_core.h): a cell's float32 score does not depend on which
// candidate won, so only scores are stored; the argmin of the few cells on the optimal
// tree is recomputed with the reference's tie rule at backtrack time.
//
// Kernels:
//   kp_counts_kernel : per-block fold counts K[h] of the block's k-mer-low cells (replaces
//                      the first-pair M/U aggregation, CV :52-55, Fit :50-53); one launch
//                      per high level, once per fold table
//   kp_dp_kernel     : the DP of every cell of one block for NL lanes (CV handle_pattern
//                      :26-78 / score_test_folds :15-20, Fit handle_pattern :31-64 / score
//                      :26-29); one launch per (high level, lane class)
//       counts : separable count tables of the block in LDS (no recurrence)
//       gather : every high-position split pair = two coalesced float4 reads of whole
//                child-block rows (HBM/L2), min-reduced
//       levels : low-position splits inside LDS, level by level, then the float64
//                single-pattern term
//       store  : the block's score rows, float4
//   kp_bt_*          : breadth-first backtrack of every lane at once: one wave per tree
//                      node recomputes the node's decision (kp_cell_decide semantics),
//                      checks it reproduces the stored score, and appends the children;
//                      kp_bt_finish sums the test -2LL along the tree in float32 (CV
//                      :158-163) and lists the leaves in the reference's order (Fit :17-24)
//   kp_codes_kernel  : argmin code of every cell (parity dumps only)
//   kp_allk_terms / kp_allk_sums : --score all_kmers (kp_allk.h; all_kmers_CV.py :8-46):
//                      every (k-mer, fold) term in parallel, then the reference's
//                      sequential float64 sum over k-mers, one thread per column
//   kp_greedy_*      : the greedy top-down partition (kp_greedy.h;
//                      greedy_penalty_plus_pseudo.py :159-196): no lattice, one tree per
//                      lane grown breadth-first from per-node nucleotide histograms
//   kp_apply_*       : a fitted partition applied to a count table (kp_apply.h): every row's
//                      one-hot word against every pattern's mask word, per-pattern uint64
//                      totals, the pairwise overlap check and the table's -2 log-likelihood
//   kp_seq_*         : k-mer context counts of a genome and its mutation sites (kp_seq.h): a
//                      streaming scan with a rolling window per thread and a histogram in LDS
//                      counters (k <= 7) or global 64-bit atomics; one thread per site; indels as
//                      breakpoint contexts on both strands, each placed within its equivalence
//                      interval, which a wave searches 64 positions per step (kp_indel.h)
//   kp_pred_*        a fitted partition taken back to the genome (kp_pred.h): a lookup table from
//                      k-mer code to pattern, the kp_seq roll in batches (kp_scan.h) with one gather per window, and
//                      per-region pattern histograms in LDS counters or global 64-bit atomics
//   kp_spec_*        every mutation type's partition in one pass (kp_spec.h): a table of 16-byte
//                      entries (one pattern per ALT slot), the kp_pred roll with one gather and up
//                      to three adds per window; typed site counting into three positive columns
//   kp_ispec_*       an indel model on both strands (kp_ispec.h): a table of 16-byte entries (the ins
//                      and the del pattern of a code and of its reverse complement), the kp_spec roll
//                      with one gather and up to four adds per breakpoint; per site, kp_indel's
//                      interval search and two table look-ups
//   kp_sim_*         a random mutation set drawn from a spectrum model (kp_sim.h): the kp_spec roll,
//                      one counter-based random number per position and an ordered two-pass
//                      compaction of the hits
//   kp_null_*        per-region null tables (kp_null.h): the same draw for many replicates at once,
//                      counted per region and replicate instead of listed
//
//   kp_coding_*      expected mutations per transcript by coding consequence (kp_coding.h): the
//                      kp_spec roll over CDS segments and splice intervals, a centre's codon from
//                      its neighbours and a per-segment record, counters per (class, pattern)
//
// One translation unit; the code lives in headers by subsystem:
//   kp_rt.h        host runtime: errors, allocation helpers, knobs, kp_ctx, kp_create
//   kp_core.h / kp_libm.h / kp_plan.h   arithmetic, logs and the host plan (shared with tests/emu)
//   kp_plan_dev.h  kp_plan, the device block list, kp_plan_*
//   kp_counts.h    kp_counts_kernel, kp_set_counts, kp_counts_*
//   kp_dp_kernel.h the sweep kernel
//   kp_bt.h        the backtrack kernels
//   kp_pass.h      launch code, score allocator, device groups, run_pass, kp_pass
//   kp_dump.h      parity dumps
//   kp_math.h      kp_math_*
//   kp_allk.h, kp_greedy.h + kp_greedy_api.h, kp_apply.h   the other scores with their drivers
//   kp_seq.h       the sequence scan, the sites kernel and the kp_seq_* sessions
//   kp_scan.h      what the genome scans below share: the aligned loads and the batch roll on the device,
//                  items, region check, uploads, table arena and timed launch on the host
//   kp_pred.h      the prediction scan, track and sites kernels and the kp_pred_* sessions
//   kp_spec.h      the spectrum table, scan, track and sites kernels, the kp_spec_* sessions and
//                  typed site counting
//   kp_sim.h       the draw of a mutation set from a spectrum model: Philox per position, the count,
//                  offsets and write kernels and kp_spec_simulate
//   kp_null.h      many replicates of that draw binned by region: the roll staged in LDS, the draw
//                  with the replicates on the lanes, and kp_spec_null
//   kp_coding.h    the genetic code and per-pair class functions, the coding scan and sites kernels,
//                  kp_spec_coding and kp_spec_coding_sites
//   kp_indel.h     breakpoint contexts of indels: the equivalence interval of a site searched 64
//                  positions per wave step, its placement and adds, kp_seq_indels
//   kp_ispec.h     an insertion and a deletion partition applied per breakpoint on both strands: the
//                  table of four ids per code, the scan, track and sites kernels, the kp_ispec_* sessions
//   kp_folds.h, kp_io.h, kp_out.h   fold sampler, count-file parser, row writer
#include "kp_rt.h"

#include "kp_allk.h"
#include "kp_apply.h"
#include "kp_core.h"
#include "kp_dp_kernel.h"
#include "kp_folds.h"
#include "kp_greedy.h"
#include "kp_greedy_api.h"
#include "kp_io.h"
#include "kp_out.h"
#include "kp_plan.h"
#include "kp_plan_dev.h"
#include "kp_counts.h"
#include "kp_bt.h"
#include "kp_pass.h"
#include "kp_dump.h"
#include "kp_math.h"
#include "kp_seq.h"
#include "kp_scan.h"
#include "kp_pred.h"
#include "kp_spec.h"
#include "kp_sim.h"
#include "kp_indel.h"
#include "kp_ispec.h"
#include "kp_null.h"
#include "kp_coding.h"
#include "kp_cnull.h"
