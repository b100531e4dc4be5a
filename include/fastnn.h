/*
 * fastnn.h -- C ABI of libfastnn_hip.so, the MI355X-native Canonical Neighbor-Net
 * agglomeration engine.
 *
 * The reference (JacobPorter/FastNeighborNet, Java) has no FFI layer; its seam for
 * this path is the abstract class NetMakerOriginal:
 *     ctor  (double[][] d, int numTaxa, int numThreads, ExecutorService pool)
 *                                                 NetMakerOriginal.java:51-56
 *     public int[] runNeighborNet()               NetMakerOriginal.java:129-162
 * as instantiated by FastNN.main for -mode Canonical (FastNN.java:324-328) and
 * called once (FastNN.java:378 / :391).  The entry points below are exactly what a
 * JNI binding of that seam needs (see INTEGRATION.md for the Java stub); plain
 * pointers and sizes only.
 *
 * All arithmetic on the path is IEEE binary64, one rounding per source-level
 * operation, no FMA contraction, in the reference's evaluation order, so the
 * circular order is bit-identical to the Java `-threads 1` result.
 *
 * Thread-safety: a handle is single-caller; different handles may be used from
 * different threads.  Functions return FNN_OK (0) or a negative fnn_status;
 * fnn_last_error() gives a thread-local message.  The library never aborts the
 * process and has NO CPU fallback: without a usable HIP device every call that
 * needs one fails with FNN_EHIP.
 */
#ifndef FASTNN_H
#define FASTNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FASTNN_ABI_VERSION 2  /* 2: fnn_sw_stats grew (route, certificate, give-up reason), FNN_ECAPACITY / FNN_EINEXACT */

typedef enum fnn_status {
    FNN_OK      = 0,
    FNN_EINVAL  = -1,  /* bad argument / matrix not symmetric, not finite, non-zero diagonal */
    FNN_ENOMEM  = -2,  /* host or device allocation failed */
    FNN_EHIP    = -3,  /* HIP runtime error or no device */
    FNN_ERCCL   = -4,  /* collective error (several GPUs: RCCL or the host callback) */
    FNN_ESTATE  = -5,  /* call sequence error (e.g. run before the matrix is set) */
    FNN_ECAPACITY = -6,/* split weights: the optimum has more positive splits than the dense factor of the block method
                          holds (nearly circular distances: O(n^2) splits) and the fall-back - CircularSplitWeights.java's
                          conjugate-gradient route - is not affordable at this size; nothing is returned
                          (FNN_SW_ALLOW_REFERENCE_ROUTE=1 takes that route anyway).
                          Relaxed mode (FNN_MODE_RELAXED): a row of the selection criterion has more than 16 tied row minima,
                          more than the search keeps per row - in practice more than 17 identical taxa, or a constant
                          matrix; no order is returned, the Canonical mode handles such input */
    FNN_EINEXACT = -7  /* split weights: weights_out IS filled, but the solver's own Kuhn-Tucker check of them exceeds
                          1e-9 of max|A^T d| (fnn_sw_stats.kkt_violation says by how much): not the certified optimum */
} fnn_status;

/* Kind of agglomeration event (NetMakerOriginal.java:462-488; special finish :343-360). */
enum { FNN_KIND_2WAY = 2, FNN_KIND_3WAY = 3, FNN_KIND_4WAY = 4, FNN_KIND_FINISH = 5 };

/* Options.  Zero-initialise, then set what you need. */
typedef struct fnn_opts {
    int32_t device;        /* HIP device ordinal (default 0) */
    int32_t validate;      /* 1: check symmetry / zero diagonal / finiteness on device before running */
    int32_t record_events; /* 1: keep the per-event trajectory (fnn_get_events) */
    int32_t force_exact_rx;/* diagnostic: 1 = always evaluate the ComputeRx sums with the exact
                              sequential-sum kernel instead of certifying the 4-candidate choice
                              from tree sums (same result; exercises the rare path) */
    int32_t disable_screen;/* 1 = always scan the fp64 matrix in full; default (0): from 4096 taxa on, events
                              with >= min(2048, n / 4) live nodes (not below 512) first stream a bf16 copy of the
                              matrix (2 bytes per entry, a quarter of the fp64 bytes) to find, within a rigorous
                              error bound, the few 32 x 512 tile units that can hold the minimum; only those are
                              rescanned in fp64 (same result) */
    int32_t lookahead;     /* events one screening pass may serve ("lookahead window"): 0 = default
                              (min(16 + n / 1024, 64) at most, and min(that, 16 + m / 512) for a window opened
                              with m live nodes: 48 at n = 32768), < 0 = off (every event scans), > 0 = that
                              many (capped at 512); same result either way */
    int32_t lookahead_pairs;/* wanted number of tracked pairs per window (0 = default 49152; the list holds 65536) */
    int32_t mode;          /* FNN_MODE_CANONICAL (0, default) or FNN_MODE_RELAXED: `-mode Relaxed` without `-additive`
                              (FastNN.java:329-338, NeighborNetLocal.java:170-264) - while more than 1024 nodes are
                              active the pair to merge is found by the randomised search for mutual row minima instead
                              of the full scan; everything else (4-candidate choice, merges, expansion) is the same */
    uint32_t relaxed_seed_lo, relaxed_seed_hi; /* seed of the Relaxed mode's generator: java.util.Random(seed) (the
                              reference draws from ThreadLocalRandom, NeighborNetLocal.java:30, which cannot be seeded;
                              with java.util.Random - the generator of the line it replaced, :27 - a run is reproducible) */
    int32_t relaxed_min_active; /* tests: the relaxed search runs while num_active > this (0 = the reference's 1024,
                              NetMakerOriginal.java:361) */
    int32_t reserved[5];
} fnn_opts;

enum { FNN_MODE_CANONICAL = 0, FNN_MODE_RELAXED = 1 };

/* One agglomeration event == one iteration of the loop of
 * NetMakerOriginal.agglomNodes (:339-393).  Same fields as the test oracle's
 * nno_event so trajectories can be compared field by field. */
typedef struct fnn_event {
    int32_t m_before;      /* num_active at loop entry */
    int32_t c_before;      /* num_clusters at loop entry */
    int32_t cx_id, cy_id;  /* Cx.id, Cy.id after the id swap (:376-380); 0 for FINISH */
    int32_t x_id, y_id;    /* nodes chosen among the <=4 candidates (:428-452) */
    int32_t kind;          /* FNN_KIND_* */
    int32_t u_id;          /* id of the node returned by agg2way/agg3way/agg4way */
    double  best;          /* scan minimum Qpq (NeighborNetCanonical.java:170-177) */
    int64_t entries;       /* E_t = m(m-1)/2 - (m-c): matrix entries the scan must read */
} fnn_event;

typedef struct fnn_stats {
    int64_t n_events;        /* agglomeration events executed */
    int64_t sum_entries;     /* sum_t E_t  (algorithmic entries; x8 = algorithmic bytes) */
    double  t_init_s;        /* initial row sums (NetMakerOriginal.initialize :164-191) */
    double  t_agglom_s;      /* agglomNodes loop, device time incl. launches */
    double  t_expand_s;      /* expandNodes on the host (:246-325) */
    double  t_total_s;       /* matrix resident on device -> order on host */
    double  t_scan_s;        /* sum of the durations of the timed k_screen launches (HIP events; 0 unless timing
                                is enabled): all of them without lookahead windows, the scheduled base scans with */
    int64_t scan_launches;   /* number of those launches */
    int64_t scan_bytes;      /* matrix bytes those launches had to stream: E_t entries at 2 B (bf16 screening
                                copy) per launch, plus the fp64 rescans of the candidate units */
    int64_t n_rx_certified;  /* events whose 4-candidate choice was certified from approximate row sums */
    int64_t n_rx_exact;      /* events that needed the exact sequential ComputeRx sums */
    int64_t n_screen_events; /* events whose scan went through the bf16 screening pass */
    int64_t n_rescan_units;  /* 32 x 512 units rescanned in fp64 over those events */
    int64_t n_base_scans;    /* events that ran a scan (all of them without lookahead windows) */
    int64_t n_window_hits;   /* events whose minimum came from an open lookahead window (no scan) */
    int64_t n_window_fails;  /* events whose window could not certify the minimum (they rescanned) */
    int64_t window_pairs;    /* tracked pairs summed over all windows */
    int64_t bytes_total;     /* matrix bytes read by ALL scan work of the run (timed or not, window items too) */
    int64_t n_handover_retries; /* window events whose per-workgroup records failed their check word on the first read
                                (the hand-over inside k_track is checked: fence + second read, then the event scans);
                                expected 0 */
    int64_t n_sweeps_exact;  /* ... whose sweep of the newest cluster's rows had to wait for its exact row sum */
    double  t_plain_s;       /* sum of the durations of the plain fp64 scan launches (k_scan; m below the screening threshold) */
    int64_t plain_launches;  /* number of those launches */
    int64_t plain_bytes;     /* 8 * E_t summed over them */
    int64_t n_stalled_events;/* launch sequences without scan kernels that found their window gone (they do nothing; the
                                host relaunches with a scan at its next look at the state) */
    int64_t n_relaxed_events;/* Relaxed mode: events whose pair came from the search for mutual row minima (the others scanned) */
} fnn_stats;

typedef struct fnn_handle fnn_handle;

/* Library / device probing. */
int32_t     fnn_abi_version(void);
const char* fnn_last_error(void);
int32_t     fnn_device_count(void);                 /* <0 on error */

/* Handle lifecycle.  n = number of taxa (ntax of NetMakerOriginal.java:52). */
int32_t fnn_create(int32_t n, const fnn_opts* opts, fnn_handle** out);
int32_t fnn_destroy(fnn_handle* h);

/* Matrix upload: rows [row0, row0+nrows) of the symmetric n x n fp64 matrix, host
 * memory, row stride ld_in doubles.  Plays the role of the `double[][] d`
 * constructor argument; the caller's buffer is never written (the reference
 * destroys its argument in place, NetMakerOriginal.java:653-656). */
int32_t fnn_set_rows(fnn_handle* h, int32_t row0, int32_t nrows, const double* rows, int64_t ld_in);
/* The same matrix from the reference's own container: the packed strict upper triangle of
 * DistancesAndNames (`double[] distances`, n(n-1)/2 entries, row-major: entry (a, b), a < b, at
 * a(n-1) - a(a-1)/2 + b - (a+1), DistancesAndNames.java:24-38).  Replaces the dense expansion of
 * FastNN.java:307-312: half the bytes cross the bus, the device mirrors the triangle itself. */
int32_t fnn_set_packed_upper(fnn_handle* h, const double* packed);
/* Same from DEVICE memory (whole matrix, row stride ld_in doubles).  The copy runs on the engine's own (non-blocking)
 * stream, which is NOT ordered against the stream that produced d_matrix: synchronise the producer (stream or device)
 * before this call.  The call returns after the copy has completed. */
int32_t fnn_set_matrix_device(fnn_handle* h, const double* d_matrix, int64_t ld_in);
/* Fill the device matrix with the synthetic generator of SURVEY.md 8(d)
 * (SplitMix64; dist 0 = uniform53, 1 = dec4), bit-identical to the host generator. */
int32_t fnn_synth(fnn_handle* h, uint64_t seed, int32_t dist);

/* The matrix as it is resident on the device (after an upload or fnn_synth, before the run consumes it), to host memory with
 * row stride ld_out doubles: what a caller needs who generated the distances on the device and wants them for the split
 * weights or the Nexus document afterwards (the reference re-parses its file for that, FastNN.java:438). */
int32_t fnn_get_matrix(fnn_handle* h, double* out, int64_t ld_out);

/* runNeighborNet (NetMakerOriginal.java:129-162): order_out has n+1 entries,
 * order_out[0] = 0, order_out[1] = 1, 1-based taxon ids in circular order; n <= 3
 * gives the identity (:133-140).  Consumes the device matrix (a new upload or
 * fnn_synth is needed before another run).  stats may be NULL. */
int32_t fnn_run(fnn_handle* h, int32_t* order_out, fnn_stats* stats);

/* Test/diagnostic stepping: fnn_begin computes the initial row sums; fnn_step
 * executes exactly one event and returns 1 (ev filled), or 0 when the loop has
 * ended; fnn_finish expands the merge stack into the order.  fnn_run ==
 * begin + step* + finish without the per-event host round trip. */
int32_t fnn_begin(fnn_handle* h);
int32_t fnn_step(fnn_handle* h, fnn_event* ev);
int32_t fnn_finish(fnn_handle* h, int32_t* order_out);

/* Trajectory of the last run (needs opts.record_events). Copies up to max_events
 * records; returns the number of events of the run (may exceed max_events). */
int64_t fnn_get_events(fnn_handle* h, fnn_event* out, int64_t max_events);

/* State inspection for parity tests.  For reference position i in
 * [0, num_active): node id, partner id (0 if none), Sx.  Arrays of length >= n. */
int32_t fnn_get_counts(fnn_handle* h, int32_t* num_active, int32_t* num_clusters, int32_t* num_nodes);
int32_t fnn_get_nodes(fnn_handle* h, int32_t* id, int32_t* nbr_id, double* Sx);
/* Sub-matrix of live nodes in reference position order: out[i*m + j] =
 * D[N[i].distID][N[j].distID], m = num_active. */
int32_t fnn_get_live_matrix(fnn_handle* h, double* out);

/* Diagnostic: one record of 5 doubles per scanned event of the last run {events done, live nodes,
 * window width W (-1: no window opened), pairs emitted, events the previous window served}; returns
 * the number of records copied (at most 8192 are kept). */
int64_t fnn_debug_window_log(fnn_handle* h, double* out, int64_t max_records);

/* Diagnostic: 100 MHz ticks (s_memrealtime) that thread 0 of the LAST-arriving tracking workgroup of k_track
 * spent, summed over the window events of the last run, in {prologue (control block, partial sums), tracked
 * pairs, sweep of the newest cluster's rows, workgroup reduction, arrival tickets, reading all workgroups'
 * records, the window's verdict, the decision tail (Cx/Cy, 4-candidate choice, merge plan)}. */
int32_t fnn_debug_event_ticks(fnn_handle* h, int64_t* out8);
/* Diagnostic (FNN_TICKS=1): the same for k_update, summed over all events: thread 0 of the workgroup of the involved
 * slots {control block, block load, phases, tail} and of the first bulk workgroup {control block, -, columns, tail}. */
int32_t fnn_debug_update_ticks(fnn_handle* h, int64_t* out8);
/* ... and the decide step inside k_track's tail: {the one round trip of loads, Cx/Cy + certified choice, merge plan,
 * symbolic replay of the micro-ops}. */
int32_t fnn_debug_decide_ticks(fnn_handle* h, int64_t* out4);
/* ... and inside the merge plan (wave 0; all decide steps of the run, k_decide's included): {the <= 4 candidates' values and the choice,
 * the chosen nodes' ids, the slot operations of the merge (swaps / agg3way plans / moves), the window's bookkeeping for the new cluster}. */
int32_t fnn_debug_plan_ticks(fnn_handle* h, int64_t* out4);
/* Diagnostic: the record the decide step leaves for k_update (packed plan + prefetched block of the involved slots), counted over
 * the events since fnn_begin: {events whose update consumed a record, ... of which took the pending exact row sum of the newest
 * cluster from the chain workgroup's word instead of the prefetch, records refused as stale (expected 0; the run fails), reserved}. */
int32_t fnn_debug_update_pre(fnn_handle* h, int64_t* out4);
/* ... and k_update per workgroup: out768[w] = sum over the events of workgroup w's start stamp, out768[256 + w] = of its end stamp,
 * out768[512 + w] = the number of events it took part in (w = 255: the workgroup of the involved slots; bulk workgroups >= 254
 * share slot 254): which workgroup ends last, and by how much. */
int32_t fnn_debug_update_wg_ticks(fnn_handle* h, int64_t* out768);
/* Relaxed mode, FNN_TICKS=1: 100 MHz ticks summed over the run in {the workgroup's row-minimum passes, their finish by
 * the control lane, the whole search kernels}, and the number of row minima computed. */
int32_t fnn_debug_relaxed_ticks(fnn_handle* h, int64_t* out4);

/* Per-launch HIP-event timing on the engine's stream (two event records per timed launch): 1 = the streaming scan
 * kernels only (bench.py's roofline figure: fnn_stats.t_scan_s / scan_launches), 2 = every kernel of the launch
 * sequences (perturbs the run a little: for an extra, untimed run), 0 = off. */
int32_t fnn_set_scan_timing(fnn_handle* h, int32_t enable);
/* With timing on: milliseconds and launches of the last run by kernel class {0 k_scan, 1 k_screen, 2 k_track,
 * 3 k_decide, 4 k_update, 5 k_emit, 6 k_resolve, 7 k_finalize}. */
int32_t fnn_get_kernel_times(fnn_handle* h, double* ms8, int64_t* launches8);
/* Several ranks, timing 2: milliseconds and calls of {0 the all-gather of a sharded base scan on the stream, 1 k_merge}. */
int32_t fnn_get_exchange_times(fnn_handle* h, double* ms2, int64_t* launches2);

/* One-call convenience == create + set_rows + run + destroy
 * (FastNN.java:326 + :378). */
int32_t fnn_canonical_order_f64(const double* D, int32_t n, int64_t ld, const fnn_opts* opts,
                                int32_t* order_out, fnn_stats* stats);

/* ---- many small problems: one call, one workgroup per problem ------------------------------------
 * `batch` Canonical runs of the same size n in one call (bootstrap replicates, per-gene matrices, sliding windows).  Problem b
 * is the n x n matrix at D + b * stride with row stride ld doubles (ld >= n, stride >= n * ld; padding is never read).
 * For 4 <= n <= fnn_batch_lds_max_n() one kernel launch per chunk runs every problem of the chunk in its own workgroup,
 * entirely out of LDS: same arithmetic contract as above, so every order, every event and every scan
 * minimum is what fnn_canonical_order_f64 gives for that matrix.  For fnn_batch_lds_max_n() < n <= fnn_batch_global_max_n()
 * and batch >= fnn_batch_global_min_batch(n) a second kernel does the same with the matrix in a per-problem working copy in
 * global memory and everything else in LDS (n_global counts them; block_threads and lds_bytes then describe that kernel);
 * the caller's matrices are never written: the host entry runs in its own upload buffer, the device entry copies each
 * problem into a working buffer of the call's (at most 2 GiB, and at least one problem, at a time).  Anything else goes,
 * problem by problem, through one fnn_handle that the call creates once (n_fallback counts them); n <= 3 gives identities
 * without touching the device; batch == 0 is FNN_OK.
 * opts: device and validate as for fnn_create - with validate set, the first problem (lowest index) whose matrix is not
 * symmetric, not finite or has a non-zero diagonal fails the whole call with FNN_EINVAL and is named in fnn_last_error();
 * mode FNN_MODE_RELAXED is accepted (it equals Canonical up to 1024 taxa); the events are recorded when events_out is given
 * (opts->record_events, which tells a handle to KEEP a trajectory for fnn_get_events, has no handle to act on here: the
 * array is the request; in the fallback the call sets it itself when events_out is given).  A problem whose kernel reached a branch that cannot be reached fails the call
 * with FNN_EHIP, named likewise.  Whatever fails, the output arrays are untouched: they are written when all problems are done.
 * orders_out: batch x (n + 1), each row as fnn_run's; events_out: NULL or batch x n records, row b holding nevents_out[b] events
 * (zero-filled behind them); nevents_out: NULL or batch.  The matrices travel in chunks of at most 2 GiB (FNN_BATCH_CHUNK=<problems>
 * overrides the chunk size, for tests; FNN_BATCH_THREADS=256|512|1024 overrides the workgroup size chosen from n, for
 * tools/batch_perf.py; FNN_BATCH_ROUTE=global sends any 4 <= n <= fnn_batch_global_max_n() and any batch >= 1 to the
 * global-memory kernel, for tests; FNN_BATCH_ROUTE=engine keeps every n above fnn_batch_lds_max_n() on the handle loop, for
 * tools/batch_perf.py).  The call runs on opts->device and leaves the caller's current HIP device as it found it.  The device variant reads D from device memory in place; like fnn_set_matrix_device it
 * is not ordered against the stream that produced D: synchronise the producer first. */
typedef struct fnn_batch_stats {
    int64_t n_problems, n_lds, n_fallback, n_events;   /* problems run in LDS / through the one-problem engine; events over all */
    int32_t lds_max_n, block_threads, lds_bytes, chunks;
    double  t_upload_s, t_kernel_s, t_total_s;
    int64_t n_global;                                   /* problems run by the global-memory kernel (was reserved[0]) */
    int64_t reserved[3];
} fnn_batch_stats;
int32_t fnn_batch_lds_max_n(void);
int32_t fnn_batch_global_max_n(void);                   /* the largest n of the global-memory route (1024) */
int64_t fnn_batch_global_min_batch(int32_t n);          /* the smallest batch that takes it by default at this n */
int32_t fnn_canonical_order_batch_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch,
                                      const fnn_opts* opts, int32_t* orders_out /* batch x (n+1) */,
                                      fnn_event* events_out /* NULL or batch x n */, int32_t* nevents_out /* NULL or batch */,
                                      fnn_batch_stats* stats /* may be NULL */);
int32_t fnn_canonical_order_batch_device_f64(const double* d_D, int32_t n, int64_t ld, int64_t stride, int64_t batch,
                                             const fnn_opts* opts, int32_t* orders_out, fnn_event* events_out,
                                             int32_t* nevents_out, fnn_batch_stats* stats);

/* ---- ragged batches: problems of DIFFERENT sizes in one call -----------
 * Per-gene matrices and sliding windows over alignments with missing taxa: problem b is the n[b] x n[b] matrix at
 * D + offsets[b] (in doubles) with row stride ld[b] (ld == NULL: ld[b] = n[b]).  offsets, n and ld are host arrays in both
 * variants; two problems may share or overlap storage; padding is never read and D is never written.  Every problem gets
 * exactly what fnn_canonical_order_batch_f64 gives it in a batch of its own size, and the contract is that call's, problem
 * by problem: n[b] <= 3 gives the identity without a device, batch == 0 is FNN_OK, opts->validate, opts->mode and
 * opts->device act alike, a negative n[b], an ld[b] below n[b] or a NULL array is FNN_EINVAL, fnn_last_error() names the
 * lowest failing problem in the CALLER's numbering (the call sorts the problems by size internally; nothing of that shows),
 * and whatever fails, the output arrays are untouched.
 * orders_out is concatenated: problem b's n[b] + 1 entries start at the sum of n[a] + 1 over a < b; events_out (NULL or
 * concatenated): problem b's n[b] records start at the sum of n[a] over a < b, nevents_out[b] events, zero-filled behind
 * them; nevents_out: NULL or batch.
 * Problems of 4 <= n[b] <= fnn_batch_lds_max_n() run one workgroup each, out of LDS, in a few launches per chunk: the call
 * sorts them into size classes (one block size and one LDS reservation per launch: at most 8, 6 with the default block
 * sizes) and starts the largest problems first.  Larger problems are grouped by size and handed to the same-size entry,
 * which picks the global-memory kernel or the one-problem engine by its own rule.  The host variant packs each chunk (at
 * most 2 GiB, FNN_BATCH_CHUNK=<problems> for tests) into one dense device image; the device variant reads D in place, with
 * 16-byte loads for a problem that is dense and 16-byte aligned, and is not ordered against the stream that produced D.
 * stats: chunks counts kernel launches, block_threads and lds_bytes describe the largest class launched, the counters are
 * summed over everything.  FNN_RAGGED_STREAMS=1..4: the streams the classes of a chunk are spread over (default: one for the orders, two for the
 * split weights, as measured). */
int32_t fnn_canonical_order_ragged_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld /* or NULL */,
                                       int64_t batch, const fnn_opts* opts, int32_t* orders_out /* sum of n[b] + 1 */,
                                       fnn_event* events_out /* NULL or sum of n[b] */, int32_t* nevents_out /* NULL or batch */,
                                       fnn_batch_stats* stats /* may be NULL */);
int32_t fnn_canonical_order_ragged_device_f64(const double* d_D, const int64_t* offsets, const int32_t* n, const int64_t* ld,
                                              int64_t batch, const fnn_opts* opts, int32_t* orders_out, fnn_event* events_out,
                                              int32_t* nevents_out, fnn_batch_stats* stats);

/* ---- several GPUs of one node (one process per GPU): ONE problem on all ranks -----------------
 * Every rank holds the whole matrix (8 GiB at n = 32768, 3 % of an MI355X) and runs the whole event chain
 * itself (the ranks stay in step because every decision is a deterministic function of identical state), so no
 * matrix row ever crosses xGMI.  All ranks must upload the same matrix and make the same calls; every rank
 * returns the same order.  What is shared out:
 *   - with lookahead windows (a screening copy exists: n >= 4096, lookahead not off): only the BASE SCANS of the
 *     windows, by screening-tile index mod world; each is followed by ONE all-gather of a fixed block per rank -
 *     16 B header + 64 candidate records of 24 B + 65536 / world tracked-pair records of 48 B - after which every
 *     rank builds the same tracked list and reduces the same candidate records;
 *   - without windows: the scan of every event, by tile index mod world, with one all-gather of <= 64 candidate
 *     records (24 B each) per rank and event.
 *
 * fnn_comm_unique_id: rank 0 creates the 128-byte RCCL id and the caller ships it to the other
 * ranks (bench.py uses torch.distributed for that).  fnn_comm_init_rccl: collective over all
 * ranks; the all-gathers then run as ncclAllGather on the engine's stream (no host round
 * trip).  rccl_path may name the librccl.so to dlopen (NULL: default search).
 * fnn_comm_init_host: test transport - the engine synchronises once per exchange and calls
 * `fn(ctx, send, recv, bytes_per_rank)` on the host, which must fill recv with every rank's
 * `send` in rank order and return 0. */
#define FNN_COMM_ID_BYTES 128
typedef int32_t (*fnn_allgather_fn)(void* ctx, const void* send, void* recv, int32_t bytes_per_rank);
int32_t fnn_comm_unique_id(uint8_t* id_out, const char* rccl_path);
/* Can this process load librccl (dlopen + the four symbols the engine uses)?  No call is made into the library: no
 * bootstrap listener is started, nothing needs tearing down.  FNN_OK or FNN_ERCCL with fnn_last_error(). */
int32_t fnn_comm_probe(const char* rccl_path);
int32_t fnn_comm_init_rccl(fnn_handle* h, int32_t world, int32_t rank, const uint8_t* id, const char* rccl_path);
int32_t fnn_comm_init_host(fnn_handle* h, int32_t world, int32_t rank, fnn_allgather_fn fn, void* ctx);

/* ---- circular split weights ------------------------------------------------
 * Non-negative least-squares weights of the n(n-1)/2 circular splits of `ordering` (the array
 * fnn_run returns: n + 1 entries, [1..n] = 1-based taxon ids in circular order) for the symmetric
 * n x n distances D (host memory, row stride ld): the unique optimum that the reference's live path
 * computes with a dense design matrix (FastNN.java:401-454), here on the implicit operators A b, A^T y
 * of CircularSplitWeights.java (2-D prefix sums) with the re-ordering of the distances restored.
 * Three routes to the same optimum: the Chepoi-Fichet closed form when it is feasible; "from below"
 * (a BLOCK active-set method: whole blocks of splits - local maxima of the multiplier - enter the free set
 * per step and every weight that is not positive leaves; the free set's normal equations, whose entries have
 * a closed form, are held as an inverse Cholesky factor that is appended to, never updated; right for
 * distances that are far from circular, where only ~2.4 n ... 3.8 n splits end up positive; 32768 taxa in
 * about a minute); CircularSplitWeights.java's own active-set / conjugate-gradient
 * method (from above) for inputs whose free set outgrows the dense factor (nearly circular metrics) - and
 * only where that route is affordable: see fnn_sw_stats.status.  weights_out has n(n-1)/2
 * entries in the index order of the reference's live path (FastNN.java:405-419): k runs over
 * (i, j), 0 <= i < j <= n-1, row-major, split k = taxa ordering[i+1 .. j] against the rest.  The
 * reference keeps the splits with weight > 1e-6 (FastNN.java:455). */
typedef struct fnn_sw_stats {
    int64_t outer_iterations; /* from below: steps (a BLOCK of splits enters the free set per step); reference method: passes of its active-set loop */
    int64_t cg_calls;         /* conjugate-gradient solves (reference method only) */
    int64_t cg_iterations;    /* ... and their iterations (each applies A and A^T once) */
    int64_t nsplits;          /* weights above 1e-6 */
    double  t_solve_s;        /* device time from the re-ordered distances to the weights */
    int64_t reserved[3];      /* [0] 1 = solved from below (block active-set method), [1] rebuilds of the factor, [2] sub-problems solved
                                 (batch kernel: [1] 0, [2] the steps that its step limit counts: entering splits plus ratio steps) */
    /* ---- ABI version 2 ---- */
    int32_t route;            /* FNN_SW_ROUTE_*: which of the three routes produced weights_out */
    int32_t certified;        /* 1 = the weights passed the solver's own Kuhn-Tucker check (kkt_violation <= 1e-9) */
    double  kkt_violation;    /* max(-min x, max |g| over x > 0, max -g over x = 0) / max|A^T d| with g = A^T (A x - d), evaluated
                                 on the device from the RETURNED weights with the implicit operators (independent of the factor) */
    double  final_threshold_rel; /* from below: the candidates' final multiplier threshold / max|A^T d|: 1e-12 unless the
                                 noise-floor rule raised it */
    int64_t n_set_aside;      /* from below: splits still set aside at termination (numerically dependent on the factor, or no
                                 measurable descent); their multipliers are covered by kkt_violation */
    int64_t capacity;         /* from below: splits the dense factor holds on this device for this n */
    int64_t free_set_peak;    /* from below: the largest number of splits the factor held */
    int32_t giveup_reason;    /* from below gave up (FNN_SW_GIVEUP_*; 0 = it did not): the reference route ran, or FNN_ECAPACITY */
    int32_t pad_;
    int64_t entered, screened_out, departed; /* from below: splits appended / dropped by the Schur-complement screening / left */
    double  t_alloc_s;        /* seconds in hipMalloc for the factor's buffers (0.1-2.7 s from box to box at 32768 taxa) */
    int64_t reserved2[4];     /* batch kernel only (0 from the one-problem solver), how often its safety net ran: splits set aside as
                                 numerically dependent on the factor [0] on a fresh append, [1] on a rebuild, [2] splits set aside
                                 because they left in the step in which they entered, [3] low 32 bits: rechecks of the splits set
                                 aside before the optimum was declared, high 32 bits: releases after progress.  n_set_aside is
                                 only what was still aside at the end */
} fnn_sw_stats;
enum { FNN_SW_ROUTE_CLOSED_FORM = 0, FNN_SW_ROUTE_FROM_BELOW = 1, FNN_SW_ROUTE_REFERENCE = 2 };
enum { FNN_SW_GIVEUP_NONE = 0, FNN_SW_GIVEUP_CAPACITY = 1,   /* the free set outgrew the dense factor */
       FNN_SW_GIVEUP_STEPS = 2,                              /* step limit (40 n + 1000) */
       FNN_SW_GIVEUP_NUMERIC = 3,                            /* BLAS / Cholesky failure */
       FNN_SW_GIVEUP_DEPARTED = 4,                           /* the departed splits outgrew their buffers */
       FNN_SW_GIVEUP_SETUP = 5 };                            /* allocation / library set-up failed */
/* Returns FNN_OK with the certified optimum; FNN_EINEXACT with weights that failed the check (from below only: the
 * reference route stops by its own rule, CG_EPSILON = 1e-8, ~1e-5 short of the optimum, and reports certified = 0 with
 * FNN_OK); FNN_ECAPACITY when the block method's factor cannot hold the free set and n is above the size up to which the
 * reference route is taken automatically (FNN_SW_REFERENCE_MAX_N, default 1024: measured in DESIGN.md section 7).  Before
 * that the block method retries with a factor of four times the capacity, up to what device memory holds (~150 000 splits).
 * FNN_EINVAL when one of the n (n - 1) / 2 distances that the ordering selects is a NaN or an infinity (checked on the device
 * before any route is chosen).  Every threshold of the solver is relative to max|A^T d|, so D -> ldexp(D, k) gives exactly
 * ldexp(weights, k) on the same route with the same counters while 2|k| + log2(n^4 max|D|^2) < 1000 (the objective is quadratic
 * in the scale and must stay a normal double). */
int32_t fnn_split_weights_f64(const double* D, int32_t n, int64_t ld, const int32_t* ordering, int32_t device,
                              double* weights_out, fnn_sw_stats* stats);
/* The same solve, returning only the weights above `threshold` (the reference's list keeps x[k] > 1e-6, FastNN.java:455-466): pairs
 * (index_out[q], weight_out[q]) in ascending live index k - the order of the reference's `splits` list -, *count_out = how many
 * there are (if it exceeds `capacity`, only the first `capacity` found are returned: call again with more room).  At 32768 taxa:
 * 77 000 pairs instead of 5.4e8 doubles (4.3 GB) over the bus.  FNN_EINEXACT / FNN_ECAPACITY as above. */
int32_t fnn_split_weights_sparse_f64(const double* D, int32_t n, int64_t ld, const int32_t* ordering, int32_t device, double threshold,
                                     int64_t* index_out, double* weight_out, int64_t capacity, int64_t* count_out, fnn_sw_stats* stats);
/* The solver keeps its large device buffers (>= 64 MiB each, ~220 GB at 32768 taxa) in a per-process pool between calls - hipMalloc of
 * them costs 0.5-4.8 s - and hands them out again to a later call of the same size; this call gives them back to the driver.  (The
 * pool is also emptied when a device allocation of the solver fails; the order engine's own 10 GiB at 32768 taxa fit beside it.) */
int32_t fnn_split_weights_release_cache(void);

/* ---- circular split weights of many small problems: one call, one workgroup per problem -----------
 * The second half of a batched Neighbor-Net run: `batch` problems of the same size n, laid out as for
 * fnn_canonical_order_batch_f64 (problem b at D + b * stride, row stride ld; ld >= n, stride >= n * ld; padding is never
 * read, D is never written), with row b of `orderings` (batch x (n + 1), host memory) what the order batch returned for
 * problem b.  weights_out: batch x n(n-1)/2, row b as fnn_split_weights_f64's weights_out for problem b.
 * For 2 <= n <= fnn_split_weights_batch_max_n() and batch >= fnn_split_weights_batch_min_batch(n) one kernel launch per
 * chunk solves every problem of the chunk in a workgroup of its own: the Chepoi-Fichet closed form where it is feasible
 * (n_closed_form), else Lawson-Hanson from below, one split per step, on an inverse Cholesky factor of the free set that is
 * appended to and never updated (n_kernel), followed by the same Kuhn-Tucker certificate as the one-problem call, computed
 * from the weights with the prefix-sum operators alone.  A problem whose free set outgrows the per-problem factor
 * (`capacity` splits: min(n(n-1)/2, 6 n); FNN_SW_BATCH_CAP=<splits> lowers it, for tests), that exceeds 40 n + 1000 steps
 * (FNN_SW_BATCH_STEPS=<steps >= 1> replaces the limit, for tests; FNN_SW_BATCH_DEP=<x>, 0 < x < 1, replaces the relative
 * threshold 1e-9 below which an appended split counts as numerically dependent on the factor and is set aside, for tests) or
 * that ends uncertified gives up inside the kernel and goes, like every problem of a call with n above the limit, through
 * fnn_split_weights_f64 (n_fallback) - nearly circular metrics take that way.  The optimum is unique, so both ways meet.
 * stats_out (NULL or batch records): route, certified, kkt_violation, outer_iterations (steps: ONE split enters per step),
 * entered, departed, n_set_aside, free_set_peak, capacity, nsplits, final_threshold_rel from the kernel for its own problems,
 * the whole record from the one-problem solver for the others.
 * batch == 0 is FNN_OK.  n < 2, a bad layout or a row of `orderings` that is not a permutation of 1..n is FNN_EINVAL, and so
 * is a NaN or an infinity among the distances that an ordering selects (found by the kernel); a one-problem solve that
 * fails with FNN_ECAPACITY or FNN_EHIP fails the call with that status; fnn_last_error() names the lowest failing problem
 * and the output arrays are untouched: they are written when all problems are done.  FNN_EINEXACT: the outputs ARE filled,
 * and at least one problem of the one-problem solver returned weights that failed its check (stats_out[b].certified).
 * Two calls on the same input give the same bits.  The workspace travels in chunks of at most 2 GiB and at least one problem
 * (workspace_bytes; FNN_BATCH_CHUNK=<problems> overrides the chunk size, for tests; FNN_BATCH_THREADS=256|512|1024 the
 * workgroup size chosen from n, for tools/splits_batch_perf.py; FNN_SW_BATCH_ROUTE=kernel sends any batch >= 1 of
 * n <= fnn_split_weights_batch_max_n() to the kernel, FNN_SW_BATCH_ROUTE=loop keeps every call on the one-problem solver).
 * fnn_split_weights_batch_min_batch(n) is the measured crossover: 1 up to 32 taxa, 4 up to 64, 8 up to
 * 96, 16 up to 128, 32 above - a workgroup takes as long for one problem as for 256, the one-problem call costs 15-37 ms.  The call runs on `device` and leaves the caller's current HIP
 * device as it found it.  The device variant reads D from device memory in place; it is not ordered against the stream that
 * produced D: synchronise the producer first. */
typedef struct fnn_sw_batch_stats {
    int64_t n_problems, n_closed_form, n_kernel, n_fallback;   /* kernel: solved from below inside the workgroup */
    int32_t max_n, block_threads, lds_bytes, chunks;
    int64_t workspace_bytes, capacity;                          /* per-call workspace; splits the per-problem factor holds */
    double  t_upload_s, t_kernel_s, t_total_s;
    int64_t reserved[4];
} fnn_sw_batch_stats;
int32_t fnn_split_weights_batch_max_n(void);
int64_t fnn_split_weights_batch_min_batch(int32_t n);   /* the smallest batch that takes the kernel by default at this n */
int32_t fnn_split_weights_batch_f64(const double* D, int32_t n, int64_t ld, int64_t stride, int64_t batch,
                                    const int32_t* orderings /* batch x (n+1) */, int32_t device,
                                    double* weights_out /* batch x n(n-1)/2 */,
                                    fnn_sw_stats* stats_out /* NULL or batch */, fnn_sw_batch_stats* stats /* may be NULL */);
int32_t fnn_split_weights_batch_device_f64(const double* d_D, int32_t n, int64_t ld, int64_t stride, int64_t batch,
                                           const int32_t* orderings, int32_t device, double* weights_out,
                                           fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats);

/* The second half of a ragged run: problems laid out as for fnn_canonical_order_ragged_f64, `orderings` (host memory)
 * concatenated as its orders_out.  weights_out is concatenated: n[b] (n[b] - 1) / 2 weights per problem, each as
 * fnn_split_weights_f64's; stats_out: NULL or batch records.  The contract is fnn_split_weights_batch_f64's, problem by
 * problem: batch == 0 is FNN_OK; n[b] < 2, an ld[b] below n[b], a NULL array or an ordering that is not a permutation is
 * FNN_EINVAL, and so is a non-finite distance; FNN_ECAPACITY and FNN_EINEXACT as there; fnn_last_error() names the lowest
 * failing problem in the caller's numbering; whatever fails but FNN_EINEXACT, the output arrays are untouched.
 * The kernel takes the problems of n[b] <= fnn_split_weights_batch_max_n() when there are at least
 * fnn_split_weights_batch_min_batch(the largest such n[b]) of them (FNN_SW_BATCH_ROUTE=kernel|loop overrides this as for the
 * same-size call), one workgroup each in at most 8 launches per chunk (4 with the default block sizes), every problem with
 * the block size and the factor capacity of the same-size call: its weights are bit for bit that call's.  Larger problems
 * and problems that give up in the kernel go through fnn_split_weights_f64 (stats->n_fallback).  stats: as above. */
int32_t fnn_split_weights_ragged_f64(const double* D, const int64_t* offsets, const int32_t* n, const int64_t* ld /* or NULL */,
                                     int64_t batch, const int32_t* orderings /* sum of n[b] + 1 */, int32_t device,
                                     double* weights_out /* sum of n[b] (n[b] - 1) / 2 */, fnn_sw_stats* stats_out /* NULL or batch */,
                                     fnn_sw_batch_stats* stats /* may be NULL */);
int32_t fnn_split_weights_ragged_device_f64(const double* d_D, const int64_t* offsets, const int32_t* n, const int64_t* ld,
                                            int64_t batch, const int32_t* orderings, int32_t device, double* weights_out,
                                            fnn_sw_stats* stats_out, fnn_sw_batch_stats* stats);

/* ---- distance matrices of bootstrap replicates from one alignment ------------
 * The first stage of a bootstrap / jackknife / sliding-window run: one alignment and per-replicate site multiplicities go
 * in, `batch` p-distance matrices come out in the layout the batch calls above read.
 * seq: n x L bytes, row i at seq + i * lds (lds >= L; padding is never read).  Byte 255 (FNN_SITE_MISSING) means "no
 * state here" (gap, N, ambiguity: the caller maps those); every other byte is a state, compared by equality only.
 * counts: batch x L uint16_t, row b at counts + b * ldc (ldc >= L): how often site s occurs in replicate b (bootstrap
 * resampling, 0 / 1 for a jackknife or a window, pattern counts of a compressed alignment).  Both are HOST arrays in both
 * variants.  For replicate b and taxa i != j, as exact integers,
 *     valid = sum_s counts[b][s] * [seq[i][s] != 255 and seq[j][s] != 255]
 *     mism  = sum_s counts[b][s] * [both present and seq[i][s] != seq[j][s]]
 * and with model FNN_DIST_P (the only one these two entries take; any other value is FNN_EINVAL here - the corrected
 * distances have entries of their own below) D_b[i][j] = D_b[j][i] =
 * (double)mism / (double)valid, one correctly rounded division; D_b[i][i] = 0.  Replicate b is written at D_out + b * stride
 * with row stride ld (ld >= n, stride >= n * ld), padding untouched.
 * FNN_EINVAL: n <= 0, L <= 0, batch < 0, lds < L, ldc < L, ld < n, stride < n * ld, a NULL array, an unknown model,
 * 127 L >= 2^31 (the counts are summed per base-128 digit in int32) - all of these before any device use -, and
 * valid == 0 for some (b, i, j): fnn_last_error() names the lowest such (b, i, j) in lexicographic order.  batch == 0 is
 * FNN_OK; n == 1 writes the single zero.
 * The host variant writes D_out only when the whole call has succeeded and works in chunks of at most 2 GiB of device
 * output (FNN_BATCH_CHUNK=<problems> overrides the chunk size, for tests).  The device variant writes D_out (device memory)
 * in place: when it FAILS THE CONTENTS OF D_out ARE UNSPECIFIED.  It has synchronised its own stream before it returns, so
 * a batch call on D_out may follow directly.  Both run on `device` and leave the caller's current HIP device as they found
 * it.  stats: digit_passes = base-128 digits of the largest count of the call (1 up to 127 - every bootstrap -, 2 up to
 * 16383, else 3); has_missing = 1: the alignment holds a byte 255 and the kernel counts `valid` per pair (otherwise it is
 * the replicate's total; FNN_DIST_FORCE_MISSING=1 takes the counting kernel anyway, for tests). */
#define FNN_SITE_MISSING 255
enum { FNN_DIST_P = 0 };
typedef struct fnn_dist_stats {
    int64_t n_problems, n_pairs, n_sites;
    int32_t digit_passes, has_missing, block_threads, chunks;
    double  t_upload_s, t_kernel_s, t_total_s;
    int64_t reserved[4];
} fnn_dist_stats;
int32_t fnn_alignment_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds,
                                          const uint16_t* counts, int64_t batch, int64_t ldc, int32_t model, int32_t device,
                                          double* D_out, int64_t ld, int64_t stride, fnn_dist_stats* stats /* may be NULL */);
int32_t fnn_alignment_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds,
                                                 const uint16_t* counts, int64_t batch, int64_t ldc, int32_t model, int32_t device,
                                                 double* d_D_out, int64_t ld, int64_t stride, fnn_dist_stats* stats);
/* ---- corrected distances: Jukes-Cantor and Kimura two-parameter ---------------------------
 * The two entries above with a model description `m` in place of `model`; everything said there holds.  With
 * m->model == FNN_DIST_P they write the same bytes as the entries above.  The counts stay exact integers; the correction
 * is a fixed sequence of fp64 operations, one rounding each, nothing fused, with a logarithm log1p' of the library's own
 * (fdlibm's algorithm in + - * / and bit operations only: the same bits on the device and on any host).
 *   FNN_DIST_JC69, k = m->states, 2 <= k <= 255 (4 for DNA, 20 for protein).  States are compared by equality as for the
 *     p-distance.  y = (double)(k mism) / (double)((k - 1) valid);  D = -(((double)(k - 1) / (double)k) * log1p'(-y)).
 *     Saturated iff k mism >= (k - 1) valid (an integer test).  FNN_EINVAL, before any device use, when the alignment holds
 *     more than k distinct bytes other than 255.
 *   FNN_DIST_K2P (m->states is ignored).  The alignment is recoded while it is copied: A a -> 0, C c -> 1, G g -> 2,
 *     T t U u -> 3, 255 stays, EVERY OTHER BYTE becomes 255 and is counted in n_recoded (and then has_missing = 1).  With
 *     ts = sum_s counts[b][s] * [both present and the two codes differ by a transition (A <-> G, C <-> T)], tv = mism - ts:
 *     y1 = (double)(2 ts + tv) / (double)valid;  y2 = (double)(2 tv) / (double)valid;
 *     D = 0.5 * (-log1p'(-y1)) + 0.25 * (-log1p'(-y2)).  Saturated iff 2 ts + tv >= valid or 2 tv >= valid.
 *   Both: mism == 0 gives +0.0, the diagonal is +0.0, the matrices are symmetric.
 * Saturated pairs: with m->on_saturation == FNN_DIST_SAT_FAIL (0) the call fails with FNN_EINVAL; fnn_last_error() names the
 * lowest (b, i, j) in lexicographic order that is EMPTY (valid == 0) or SATURATED and says which; the host output is
 * untouched.  With FNN_DIST_SAT_CAP the entry becomes m->cap (finite, > 0) and n_saturated_problems counts the replicates
 * that had such a pair; an empty pair still fails the call.
 * FNN_EINVAL before any device use, beyond the list above: m == NULL, an unknown model or policy, states outside 2 ... 255
 * for JC69, too many distinct states, cap not finite or <= 0 under FNN_DIST_SAT_CAP.  m->reserved is 0 (equal rates) or selects gamma-distributed
 * rates (further below). */
enum { FNN_DIST_JC69 = 1, FNN_DIST_K2P = 2 };
enum { FNN_DIST_SAT_FAIL = 0, FNN_DIST_SAT_CAP = 1 };
typedef struct fnn_dist_model {
    int32_t model, states, on_saturation, reserved;
    double  cap;
} fnn_dist_model;
typedef struct fnn_dist_model_stats {
    fnn_dist_stats base;
    int64_t n_recoded, n_saturated_problems;
    int64_t reserved[2];
} fnn_dist_model_stats;
int32_t fnn_alignment_distances_model_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds,
                                                const uint16_t* counts, int64_t batch, int64_t ldc, const fnn_dist_model* m,
                                                int32_t device, double* D_out, int64_t ld, int64_t stride,
                                                fnn_dist_model_stats* stats /* may be NULL */);
int32_t fnn_alignment_distances_model_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds,
                                                       const uint16_t* counts, int64_t batch, int64_t ldc,
                                                       const fnn_dist_model* m, int32_t device, double* d_D_out, int64_t ld,
                                                       int64_t stride, fnn_dist_model_stats* stats);
/* ---- the 4 x 4 table of state pairs: F81, F84, TN93, LogDet and the table itself -----------------
 * Four more values of m->model, numbered from 16 (the family of models on the table; 3 ... 15 stay unknown), for all entries that take a fnn_dist_model (the two above and the bootstrap entries below;
 * m->states is ignored, m->reserved is the rates, below).  The alignment is recoded exactly as for K2P (n_recoded, has_missing).  For
 * i < j, with code_i the code of the LOWER-numbered taxon, as exact integers
 *     F[s][t] = sum_site counts[b][site] * [code_i == s and code_j == t]      (s, t in A 0, C 1, G 2, T 3)
 *     v = sum F;  r_s = sum_t F[s][t];  c_t = sum_s F[s][t];  n_s = r_s + c_s;  mism = v - trace F
 *     ts1 = F[A][G] + F[G][A];  ts2 = F[C][T] + F[T][C];  tv = mism - ts1 - ts2
 * and, in fp64 with one rounding per written operation (nothing fused), the PAIR's base frequencies
 *     g_s = (double)n_s / (double)(2 v);  gR = gA + gG;  gY = gC + gT
 * (frequencies given by the caller or taken over the whole alignment are not offered).  log1p' and log' are the library's
 * own (fdlibm's algorithms in + - * / and bit operations: the same bits on the device and on any host).
 *   FNN_DIST_F81     sq = ((gA gA + gC gC) + gG gG) + gT gT;  E = 1 - sq;  p = (double)mism / (double)v;  y = p / E;
 *                    D = -(E * log1p'(-y))
 *   FNN_DIST_F84     ct = gC gT;  ag = gA gG;  A = ct / gY + ag / gR;  B = ct + ag;  C = gR gY;  A2 = 2 A;
 *                    P = (double)(ts1 + ts2) / (double)v;  Q = (double)tv / (double)v;
 *                    y1 = P / A2 + ((A - B) Q) / (A2 C);  y2 = Q / (2 C);
 *                    D = -(A2 * log1p'(-y1)) + (2 ((A - B) - C)) * log1p'(-y2)
 *   FNN_DIST_TN93    k1 = ((2 gA) gG) / gR;  k2 = ((2 gT) gC) / gY;
 *                    k3 = 2 ((gR gY - ((gA gG) gY) / gR) - ((gT gC) gR) / gY);
 *                    P1 = (double)ts1 / (double)v;  P2 = (double)ts2 / (double)v;  Q = (double)tv / (double)v;
 *                    y1 = P1 / k1 + Q / (2 gR);  y2 = P2 / k2 + Q / (2 gY);  y3 = Q / (2 (gR gY));
 *                    D = (-(k1 * log1p'(-y1)) - k2 * log1p'(-y2)) - k3 * log1p'(-y3)
 *   FNN_DIST_LOGDET  m[s][t] = (double)F[s][t] / (double)v;  det = ((m00 C0 - m01 C1) + m02 C2) - m03 C3, Ck the 3 x 3
 *                    determinant of rows 1 ... 3 without column k, (a (e i - f h) - b (d i - f g)) + c (d h - e g) for
 *                    the rows a b c / d e f / g h i;  ls = the sum over s = A, C, G, T in turn, from 0.0, of
 *                    (log'((double)r_s / (double)v) + log'((double)c_s / (double)v));
 *                    D = -(0.25 * (log'(det) - 0.5 * ls)).  The determinant is not exact; it is the same everywhere.
 * Per pair, in this order: v == 0 is EMPTY (NaN; the call fails under both policies, as above); mism == 0 gives +0.0;
 * DEGENERATE by integer tests - F84, TN93: some n_s == 0; LogDet: some r_s == 0 or c_s == 0; F81: never -; SATURATED when some
 * y is not below 1.0 (!(y < 1.0) on the computed double) or LogDet's computed determinant is not above 0.  Degenerate and
 * saturated pairs follow m->on_saturation alike: FNN_DIST_SAT_FAIL fails the call and fnn_last_error() names the lowest
 * (b, i, j) that is empty, degenerate or saturated and says which; FNN_DIST_SAT_CAP stores m->cap and counts the replicate in
 * n_saturated_problems.  D[i][j] and D[j][i] are one value, computed on the table of i < j. */
enum { FNN_DIST_F81 = 16, FNN_DIST_F84 = 17, FNN_DIST_TN93 = 18, FNN_DIST_LOGDET = 19 };  /* 16 ...: the models of the table; 3 ... 15 are unknown */
/* ---- gamma-distributed rates across sites -----------------------------------------------------
 * The sequences above assume one rate for all sites.  m->reserved says otherwise: FNN_DIST_RATES_EQUAL (0, everything above)
 * or FNN_DIST_RATES_GAMMA (1): then `m` MUST POINT AT THE FIRST MEMBER OF A fnn_dist_model_rates, whose `shape` is the
 * shape parameter alpha > 0 of the gamma distribution (mean 1) and whose reserved[3] are 0.  All entries that take a
 * fnn_dist_model take it, the bootstrap entries on both draw routes.  For alpha > 0, with expm1' the library's own e^x - 1
 * (fdlibm's algorithm in + - * / and bit operations, like log1p'),
 *     g(y):  l = log1p'(-y);  t = (-l) / alpha;  e = expm1'(t);  g = alpha * e          (= alpha ((1 - y)^(-1/alpha) - 1))
 * stands in place of -ln(1 - y): in the five sequences every log1p'(-y) becomes -g(y), everything else - the coefficients, the
 * order of the sums, the signs, one rounding per written operation - stays:
 *   FNN_DIST_JC69    D = -(((double)(k - 1) / (double)k) * (-g(y)))
 *   FNN_DIST_K2P     D = 0.5 * (-(-g(y1))) + 0.25 * (-(-g(y2)))
 *   FNN_DIST_F81     D = -(E * (-g(y)))
 *   FNN_DIST_F84     D = -(A2 * (-g(y1))) + (2 ((A - B) - C)) * (-g(y2))
 *   FNN_DIST_TN93    D = (-(k1 * (-g(y1))) - k2 * (-g(y2))) - k3 * (-g(y3))
 * with y, y1, y2, y3 and the coefficients as above (the gamma distances of Jin and Nei and of Tamura and Nei).  The order of
 * the per-pair tests is unchanged - empty, mism == 0 gives +0.0, degenerate, saturated - and a pair is ALSO SATURATED when
 * some e is not finite (!(e < inf)): a small alpha has pushed t over expm1's overflow threshold 709.78...  Such a pair
 * follows m->on_saturation like the others.
 * FNN_EINVAL before any device use, with the field named: m->reserved other than 0 or 1; shape not finite or <= 0; a non-zero
 * entry of reserved[3]; FNN_DIST_RATES_GAMMA with FNN_DIST_P or FNN_DIST_LOGDET (neither has a gamma form).  With
 * FNN_DIST_RATES_EQUAL every entry writes the bytes described above and reads sizeof(fnn_dist_model) bytes of `m` only. */
enum { FNN_DIST_RATES_EQUAL = 0, FNN_DIST_RATES_GAMMA = 1 };
typedef struct fnn_dist_model_rates {
    fnn_dist_model base;   /* base.reserved = FNN_DIST_RATES_GAMMA; pass &base */
    double  shape;
    double  reserved[3];
} fnn_dist_model_rates;
/* The tables themselves, as integers: entry (b, i, j, s, t) at F_out + b * stride + (i * ld + j) * 16 + 4 * s + t for ALL i != j
 * (the block at (j, i) is the transposed table: there code_i is the row again), 16 zeros at i == j.  ld >= n and
 * stride >= 16 * n * ld; everything else - the recoding, layout of the inputs, chunks, host output written only on success,
 * the device variant's in-place output, the argument checks before any device use - is as for the entries above.  No
 * table fails the call: an empty pair is 16 zeros. */
int32_t fnn_alignment_pair_counts_batch_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const uint16_t* counts,
                                            int64_t batch, int64_t ldc, int32_t device, int64_t* F_out, int64_t ld,
                                            int64_t stride, fnn_dist_model_stats* stats /* may be NULL */);
int32_t fnn_alignment_pair_counts_batch_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds,
                                                   const uint16_t* counts, int64_t batch, int64_t ldc, int32_t device,
                                                   int64_t* d_F_out, int64_t ld, int64_t stride, fnn_dist_model_stats* stats);
/* Reproducible bootstrap multiplicities, host only (no device needed): replicate b draws k = 0 ... L - 1 and increments
 * site floor(x L / 2^64) (the high half of the 128-bit product), x = the (b L + k)-th output of SplitMix64 for `seed`
 * (z = seed + (b L + k + 1) * 0x9E3779B97F4A7C15, then the usual two multiply-xorshift rounds).  counts_out: batch x L,
 * dense.  A count above 65535 is FNN_EINVAL. */
int32_t fnn_bootstrap_counts(int64_t L, int64_t batch, uint64_t seed, uint16_t* counts_out /* batch x L */);
/* ---- bootstrap replicates drawn on the device ------------------------------------------------
 * The model entries above for the counts of a bootstrap, without the counts: `batch` counts ALL problems of the call; the
 * first `lead` of them (0 or 1) are the original data, every site counted once; problem b >= lead is replicate b - lead of
 * fnn_bootstrap_counts(L, batch - lead, seed, ...).  D_out receives the same bytes as
 * fnn_alignment_distances_model_batch[_device]_f64 writes on those counts (with lead == 1: an all-ones row in front), for
 * every model and both saturation policies, and everything said there holds with b in this call's numbering: layout,
 * chunks, host output written only on success, K2P's recoding, the lowest empty or saturated (b, i, j) named, the argument
 * checks before any device use.  FNN_EINVAL beyond those: lead outside 0 ... 1 or above batch.
 * Up to fnn_bootstrap_draw_max_sites() sites (32768: two bytes of a workgroup's 64 KiB of LDS per site) a kernel draws every
 * replicate's row of the digit planes where the distance kernel reads it: the alignment is the only upload, and of the
 * counts one word per chunk - the largest - comes back.  Longer alignments are drawn on the host (fnn_bootstrap_counts)
 * and go the way of the counts entries.  FNN_DRAW_ROUTE=device|host overrides the choice (tests); `device` above the limit
 * is FNN_EINVAL before any device use.  FNN_DIST_FORCE_DIGITS=2|3 makes any of the distance calls use at least that many
 * digit planes (tests; the result does not change).
 * stats: model = what the model entries report; draw_route; max_count = the largest multiplicity of the call; t_draw_s =
 * the draw kernel's time, part of t_total_s and of no other field. */
enum { FNN_DRAW_DEVICE = 0, FNN_DRAW_HOST = 1 };
typedef struct fnn_boot_stats {
    fnn_dist_model_stats model;
    int32_t draw_route, max_count;
    double  t_draw_s;
    int64_t reserved[4];
} fnn_boot_stats;
int32_t fnn_bootstrap_distances_batch_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed,
                                          int64_t lead, const fnn_dist_model* m, int32_t device,
                                          double* D_out, int64_t ld, int64_t stride, fnn_boot_stats* stats /* may be NULL */);
int32_t fnn_bootstrap_distances_batch_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, int64_t batch, uint64_t seed,
                                                 int64_t lead, const fnn_dist_model* m, int32_t device,
                                                 double* d_D_out, int64_t ld, int64_t stride, fnn_boot_stats* stats);
int32_t fnn_bootstrap_draw_max_sites(void);
/* ---- site ranges: per-gene matrices and sliding windows without a counts matrix -----------------
 * The model and the table entries above for problems that are contiguous runs of sites: problem b is the alignment restricted
 * to the sites starts[b] <= s < ends[b] (half-open; HOST arrays of `batch` int64_t in both variants) - a gene of a
 * concatenated alignment, one window of a scan along a genome.  Each entry writes the same bytes as its counts entry
 * (fnn_alignment_distances_model_batch[_device]_f64, fnn_alignment_pair_counts_batch[_device]_i64) writes on
 *     counts[b][s] = [starts[b] <= s < ends[b]]
 * for every model, both saturation policies and gamma rates, and everything said there holds: layout, chunks and
 * FNN_BATCH_CHUNK, host output written only on success, the device variant's in-place output and synchronised stream, K2P's
 * recoding with n_recoded and has_missing, FNN_DIST_FORCE_MISSING, n == 1, batch == 0, 127 L < 2^31, all argument checks
 * before any device use; a failing call fails with the same status and fnn_last_error() names the same lowest (b, i, j) and
 * the same kind (empty, degenerate, saturated).  No counts exist anywhere: the kernel makes its 0/1 operand from the two
 * bounds, the uploads per chunk are the bounds and one span per 16 ranges, and the kernel walks, for each TILE of 16
 * consecutive ranges in the caller's order, only the 64-site blocks from floor64(the lowest start) to ceil64(the highest end)
 * of the tile's non-empty ranges.  Ranges may overlap, nest, repeat and come in any order: the order changes the cost (ranges
 * that lie close together belong next to each other), never a byte.
 * FNN_EINVAL beyond the lists above, before any device use: a NULL starts or ends; a range outside 0 <= start <= end <= L,
 * and fnn_last_error() names the lowest such b.  An empty range (start == end) is no argument error: it is the all-zero row
 * of the counts and behaves as that row does - every pair of it is empty.
 * stats: model = what the counts entry reports (digit_passes is 1); n_site_blocks = the 64-site blocks walked, summed over the
 * call's tiles of 16 consecutive ranges (a chunk starts a new tile); n_site_blocks_dense = what the counts entries walk,
 * ceil(batch / 16) * round_up(L, 64) / 64.  Their ratio tells what an unfortunate order of the ranges costs. */
typedef struct fnn_range_stats {
    fnn_dist_model_stats model;
    int64_t n_site_blocks, n_site_blocks_dense;
    int64_t reserved[4];
} fnn_range_stats;
int32_t fnn_alignment_distances_ranges_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts,
                                           const int64_t* ends, int64_t batch, const fnn_dist_model* m, int32_t device,
                                           double* D_out, int64_t ld, int64_t stride, fnn_range_stats* stats /* may be NULL */);
int32_t fnn_alignment_distances_ranges_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts,
                                                  const int64_t* ends, int64_t batch, const fnn_dist_model* m, int32_t device,
                                                  double* d_D_out, int64_t ld, int64_t stride, fnn_range_stats* stats);
int32_t fnn_alignment_pair_counts_ranges_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts,
                                             const int64_t* ends, int64_t batch, int32_t device, int64_t* F_out, int64_t ld,
                                             int64_t stride, fnn_range_stats* stats /* may be NULL */);
int32_t fnn_alignment_pair_counts_ranges_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts,
                                                    const int64_t* ends, int64_t batch, int32_t device, int64_t* d_F_out,
                                                    int64_t ld, int64_t stride, fnn_range_stats* stats);
/* ---- bootscan: bootstrap replicates inside every site range ----------------------------------------
 * The two families above at once: `windows` ranges [starts[w], ends[w]) with 0 <= start <= end <= L (HOST arrays of `windows`
 * int64_t in every variant), `replicates` = R >= 0 bootstrap replicates of each range alone, and lead = 0 or 1 problems of
 * original data in front of them.  With P = R + lead the call has windows * P problems, window-major: problem p belongs to
 * window w = p / P and is number q = p % P of it.
 *   q < lead:   the window's original data, counts[s] = [starts[w] <= s < ends[w]].
 *   otherwise:  replicate r = q - lead of window w.  With width = ends[w] - starts[w] and seed_w = the w-th output of SplitMix64
 *               for `seed` in fnn_bootstrap_counts' convention (z = seed + (w + 1) * 0x9E3779B97F4A7C15, then the two
 *               multiply-xorshift rounds), draw k = 0 ... width - 1 is x = output r * width + k of SplitMix64 for seed_w and
 *               increments site starts[w] + floor(x * width / 2^64): row r of fnn_bootstrap_counts(width, R, seed_w) placed at
 *               columns starts[w] ..., zero elsewhere.
 * The seed of a window depends on w and not on its bounds: repeated identical ranges get different replicates.  The problems of
 * window w are, bit for bit, what fnn_bootstrap_distances_batch_f64 gives for the slice seq[:, starts[w]:ends[w]] with
 * (R + lead, seed_w, lead).  An empty window is P all-zero rows: every pair of them is empty, as with the range entries.
 * fnn_bootscan_counts (host only, no device) writes rows first ... first + count - 1 of those counts, count x L uint16_t, so
 * that no caller needs the whole windows * P x L array.  FNN_EINVAL: L <= 0, windows or replicates < 0, a NULL array, a range
 * outside 0 <= start <= end <= L (fnn_last_error() names the lowest such w), lead outside 0 ... 1, a slice outside
 * 0 ... windows * P, a count above 65535.
 * Each distance entry writes the same bytes as its counts entry (fnn_alignment_distances_model_batch[_device]_f64,
 * fnn_alignment_pair_counts_batch[_device]_i64) writes on those counts, for every model, both saturation policies and gamma
 * rates, and everything said there holds with p in this call's numbering: layout, chunks and FNN_BATCH_CHUNK (a chunk boundary
 * may fall inside a window), host output written only on success, the device variant's in-place output and synchronised stream,
 * K2P's recoding, FNN_DIST_FORCE_MISSING, n == 1, batch == 0 (no window, or P == 0), 127 L < 2^31, all argument checks before
 * any device use - among them the checks of fnn_bootscan_counts -; a failing call fails with the same status and
 * fnn_last_error() names the same lowest (b, i, j) and the same kind.
 * Routes.  While every window's padded span ceil64(end) - floor64(start) is at most fnn_bootstrap_draw_max_sites(), a kernel
 * draws every problem's row of ONE digit plane, only as long as that span, where the distance kernel reads it, and the distance
 * kernel walks one window's span against up to 64 (tables: 32) of that window's rows: the uploads per chunk are one table entry
 * per window and per such group of rows, and of the counts one word per chunk - the largest - comes back.  A chunk whose
 * largest count exceeds 127 (or every chunk under FNN_DIST_FORCE_DIGITS=2|3) is computed from fnn_bootscan_counts on the host
 * through the counts entries' own path instead (n_host_chunks); so is the whole call when a window is wider than the limit or
 * under FNN_DRAW_ROUTE=host (boot.draw_route = FNN_DRAW_HOST; n_host_chunks stays 0), with at most 256 MiB of counts at a time.
 * FNN_DRAW_ROUTE=device above the limit is FNN_EINVAL before any device use.  All routes give the same bytes.
 * stats: boot = what the bootstrap entries report (max_count, t_draw_s; digit_passes is the largest of any chunk); n_windows;
 * n_site_blocks = the 64-site blocks walked, summed over every 16 rows of every group (rows of the host route walk the whole
 * alignment); n_site_blocks_dense = what the counts entries walk, ceil(problems / 16) * round_up(L, 64) / 64. */
typedef struct fnn_scan_stats {
    fnn_boot_stats boot;
    int64_t n_windows;
    int64_t n_site_blocks, n_site_blocks_dense;
    int64_t n_host_chunks;
    int64_t reserved[4];
} fnn_scan_stats;
int32_t fnn_bootscan_counts(int64_t L, const int64_t* starts, const int64_t* ends, int64_t windows, int64_t replicates,
                            int64_t lead, uint64_t seed, int64_t first, int64_t count, uint16_t* counts_out /* count x L */);
int32_t fnn_bootscan_distances_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts,
                                   const int64_t* ends, int64_t windows, int64_t replicates, uint64_t seed, int64_t lead,
                                   const fnn_dist_model* m, int32_t device, double* D_out, int64_t ld, int64_t stride,
                                   fnn_scan_stats* stats /* may be NULL */);
int32_t fnn_bootscan_distances_device_f64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts,
                                          const int64_t* ends, int64_t windows, int64_t replicates, uint64_t seed, int64_t lead,
                                          const fnn_dist_model* m, int32_t device, double* d_D_out, int64_t ld, int64_t stride,
                                          fnn_scan_stats* stats);
int32_t fnn_bootscan_pair_counts_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts,
                                     const int64_t* ends, int64_t windows, int64_t replicates, uint64_t seed, int64_t lead,
                                     const fnn_dist_model* m /* ignored; may be NULL */, int32_t device, int64_t* F_out,
                                     int64_t ld, int64_t stride, fnn_scan_stats* stats /* may be NULL */);
int32_t fnn_bootscan_pair_counts_device_i64(const uint8_t* seq, int32_t n, int64_t L, int64_t lds, const int64_t* starts,
                                            const int64_t* ends, int64_t windows, int64_t replicates, uint64_t seed,
                                            int64_t lead, const fnn_dist_model* m, int32_t device, int64_t* d_F_out,
                                            int64_t ld, int64_t stride, fnn_scan_stats* stats);

/* ---- split support: how often each split occurs among many problems ---------
 * The last stage of a bootstrap run: the orderings and split weights of `batch` problems over ONE taxon set go in, one
 * table of the distinct splits comes out, each with the number of problems that hold it and the sum of its weights there.
 * orderings: batch x (n + 1), host memory, row b as the order batch returns it ([1..n] a permutation of 1..n).  weights:
 * batch x n(n-1)/2, dense, row b in the index order of fnn_split_weights_f64 (k <-> (i, j), 0 <= i < j <= n - 1, row-major;
 * split k of problem b = taxa orderings[b][i+1 .. j] against the rest); host memory, or device memory for the _device_
 * variant, which is not ordered against the stream that produced the weights: synchronise the producer first.
 * A record (b, k) COUNTS iff weights[b][k] > threshold in IEEE arithmetic (a NaN never counts; the reference keeps
 * x > 1e-6).  Its KEY is the split as an n-bit set, bit t - 1 for taxon t, of the side that does NOT contain taxon 1, in
 * words = ceil(n / 64) uint64_t, word 0 = taxa 1 ... 64, unused high bits zero.  Within one problem distinct k have
 * distinct keys, so a problem holds a split at most once.
 * The table has S rows, one per distinct key among the counting records of ALL problems, in order of first appearance
 * (ascending (b, k) of the lowest counting record with that key): keys_out[s * words ...], first_b_out[s], first_k_out[s],
 * counts_out[s] = the number of problems b >= lead that hold the split, weight_sum_out[s] = ((0 + w_b1) + w_b2) + ... over
 * exactly those problems in ascending b, fp64, one rounding per addition (the sequential sum).  The first `lead` problems
 * define rows - which therefore come first - but are not tallied: with lead = 1 and the original data as problem 0 the rows
 * with first_b == 0 are the reference network's splits in its own order, each with its bootstrap support; rows that only
 * lead problems hold have count 0 and sum +0.0.  lead = 0: the plain consensus tally.
 * *count_out = S.  When S > capacity the first `capacity` rows are filled and the status is still FNN_OK (call again with
 * more room); with capacity == 0 the five output arrays may be NULL.  Outputs are written only when the whole call has
 * succeeded.  Two calls on the same input give the same bytes, whatever the chunking or the route.
 * FNN_EINVAL, all before any device use: a NULL array, n < 2, n > fnn_split_support_max_n(), batch < 0, lead < 0 or
 * lead > batch, a NaN threshold, capacity < 0, a row of `orderings` that is not a permutation of 1..n (fnn_last_error()
 * names the lowest such b).  batch == 0 is FNN_OK with S = 0.  The call runs on `device` and leaves the caller's current
 * HIP device as it found it.
 * Routes (stats->route): FNN_SUPPORT_ROUTE_KERNEL - per chunk of problems (at most 2 GiB of weights; FNN_BATCH_CHUNK=<problems>
 * overrides, for tests; tallies and sums carry across chunks) a sequence of kernels: count the records, emit them in
 * (b, k) order with their keys into a hash table of 63-bit key hashes, compare every record's full key with the key of
 * its slot's first record, number the rows by a scan, scatter the tallied records into per-row segments, put each segment
 * in ascending b by rank and add it up in order.  No float atomics; kernel boundaries are the only synchronisation.  Two
 * distinct keys with one hash are detected, never resolved silently: the chunk is repeated with another hash seed
 * (hash_retries), and after 3 repeats the call takes FNN_SUPPORT_ROUTE_HOST - the same table from an ordered map in plain
 * C++ on the host (the device variant downloads the weights for it) -, which also serves calls below
 * fnn_split_support_min_work() in batch * n * n (the measured crossover).  For tests:
 * FNN_SUPPORT_ROUTE=kernel|host overrides the choice; FNN_SUPPORT_HASH_BITS=<1..64> keeps only that many bits of the hash,
 * so that distinct keys collide, the repeats run out and the host route takes over. */
enum { FNN_SUPPORT_ROUTE_KERNEL = 0, FNN_SUPPORT_ROUTE_HOST = 1 };
typedef struct fnn_support_stats {
    int64_t n_problems, n_records, n_splits;   /* n_records: counting records; n_splits: S */
    int32_t words, route, hash_retries, chunks;
    int64_t table_slots;                       /* hash slots of the largest chunk (a power of two >= 2 x its records) */
    double  t_upload_s, t_kernel_s, t_total_s;
    int64_t reserved[4];
} fnn_support_stats;
int32_t fnn_split_support_max_n(void);     /* 1024: 16 words; the limit of the batched order kernels */
int64_t fnn_split_support_min_work(void);  /* the smallest batch * n * n that takes the kernels by default */
int32_t fnn_split_support_f64(int32_t n, int64_t batch, const int32_t* orderings /* batch x (n+1) */,
                              const double* weights /* batch x n(n-1)/2 */, double threshold, int64_t lead, int32_t device,
                              uint64_t* keys_out /* capacity x words */, int64_t* first_b_out, int64_t* first_k_out,
                              int64_t* counts_out, double* weight_sum_out, int64_t capacity, int64_t* count_out,
                              fnn_support_stats* stats /* may be NULL */);
int32_t fnn_split_support_device_f64(int32_t n, int64_t batch, const int32_t* orderings, const double* d_weights,
                                     double threshold, int64_t lead, int32_t device, uint64_t* keys_out, int64_t* first_b_out,
                                     int64_t* first_k_out, int64_t* counts_out, double* weight_sum_out, int64_t capacity,
                                     int64_t* count_out, fnn_support_stats* stats);
/* Host only, no device: the keys of the splits k[0 .. count) of one ordering (n + 1 entries), keys_out: count x
 * ceil(n / 64) words, as defined above.  FNN_EINVAL: n < 2, count < 0, a NULL array with count > 0, an ordering that is
 * not a permutation, a k outside 0 ... n(n-1)/2 - 1. */
int32_t fnn_split_keys(int32_t n, const int32_t* ordering, const int64_t* k, int64_t count, uint64_t* keys_out);

/* Diagnostic: the exact block-parallel evaluation of the sequential fp64 sum
 * (((0 + b[0]) + b[1]) + ...) used for ComputeRx / u.Sx (NetMakerOriginal.java:551-560,
 * :532), run on an arbitrary host buffer.  ept = addends per thread (32, fixed by the
 * buffer layout); guard_bits != 0 in production, 0 to provoke the fallback paths.  stats4 (may be NULL)
 * = {runs applied, chunks added one by one, rejected runs, rejected chunks}. */
int32_t fnn_test_chain_sum(int32_t device, const double* host_buf, int32_t m, int32_t guard_bits,
                           int32_t ept, double* out, int32_t* stats4);
/* Diagnostic: sums of fewer addends than this take the short form (one wave, strictly in order; no records, so stats4 is
 * all zero); from this size on the record form. */
int32_t fnn_test_chain_short_below(void);

/* Device-side read-only streaming probe: reads `bytes` bytes `reps` times and
 * returns the achieved GB/s (the "measured stream" line next to the nominal
 * 8 TB/s peak). */
int32_t fnn_stream_probe(int32_t device, int64_t bytes, int32_t reps, double* gbps_out);

#ifdef __cplusplus
}
#endif
#endif /* FASTNN_H */
