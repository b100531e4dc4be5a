// fnn_support.h -- split support: the distinct splits of many problems over one taxon set, each with the number of problems
// that hold it and the sequential sum of its weights: the per-thread steps of the kernels of
// fnn_support.hip and the host side of fnn_split_support[_device]_f64, both shared with the CPU driver
// (tests/emu/fnn_support_emu.cpp) the way fnn_dist.h is; the host route (an ordered map) and fnn_split_keys.
//
// One chunk of problems on the kernel route, every step a launch of its own (kernel boundaries are the only
// synchronisation: no spin, no lane waits for another lane, no float atomics):
//   count    one workgroup per problem: the counting records (w > threshold) of the problem, an integer atomic add
//   (host)   prefix over the problems: record ids are ascending in (b, k); the hash table gets >= 2 slots per record
//   emit     one workgroup per problem: the ordering and the prefix sets P[p] = taxa at positions 1 ... p in LDS; tiles of
//            256 indices k in order, a ballot gives every counting record its id; key = P[j] ^ P[i], complemented when
//            it holds taxon 1; the key's hash goes into an open-addressing table by 64-bit compare-and-swap (a lane never
//            waits: it takes the slot, finds its own hash there, or moves on); an unsigned atomic min leaves the lowest
//            record id in the slot, an integer atomic add the number of tallied problems
//   verify   one thread per record: its full key against the key of its slot's first record; a difference is a true
//            collision of two keys on all hash bits and sets a flag (the host repeats the chunk with another seed)
//   scan     exclusive scan of the "first record" flags (two launches around a host prefix of the tile sums): the chunk's
//            rows in order of first appearance
//   rows     the first records write their row: key, (b, k), tally
//   (host)   the chunk's rows meet the rows of earlier chunks: global row ids and the partial sums to start from
//   scan     exclusive scan of the tallies: per-row segments
//   scatter  the tallied records go into their row's segment (an integer atomic cursor: arbitrary order inside)
//   rank     one thread per segment entry: its rank by b (a problem holds a split at most once, so b is unique in a
//            segment) is its place in the sorted segment
//   sum      one thread per row adds its sorted segment to the row's partial sum, in order
#ifndef FNN_SUPPORT_H
#define FNN_SUPPORT_H

#include <stdint.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "fnn_small.h"  // batch_chunk (FNN_BATCH_CHUNK), round_up; fnn_engine.h: fail, now_s, the FNN_* codes; fnn_core.h: splitmix64_at

namespace fnn {

constexpr int32_t SUP_MAX_N = 1024;        // 16 words; P[0 ... n] of 16 words is 131 200 bytes of the 160 KiB of LDS
constexpr int32_t SUP_THREADS = 256;       // every launch
constexpr int32_t SUP_WAVES = SUP_THREADS / 64;
constexpr int32_t SUP_SCAN_PER_THREAD = 4;
constexpr int32_t SUP_SCAN_TILE = SUP_THREADS * SUP_SCAN_PER_THREAD;
constexpr int32_t SUP_RETRIES = 3;         // repeats of a chunk with another seed before the call takes the host route
constexpr int64_t SUP_MIN_WORK = 262144;   // batch * n * n from which the kernel route is the default (measured crossover: DESIGN.md section 15)
constexpr uint64_t SUP_SEED = 0x53504C4954535550ull;
constexpr uint64_t SUP_USED = 1ull << 63;  // set in every stored hash: 0 is the empty slot

enum { SUP_K_COUNT = 0, SUP_K_EMIT, SUP_K_VERIFY, SUP_K_SCAN_SUMS, SUP_K_SCAN_APPLY, SUP_K_ROWS, SUP_K_SCATTER, SUP_K_RANK, SUP_K_SUM };

struct SupArgs {
    // the chunk
    const int32_t* ord;    // cnt x (n + 1)
    const double* w;       // cnt x K
    int32_t n, words;
    int64_t K, cnt, b0, lead;
    double thr;
    // records, ascending in (b, k)
    uint32_t* reccnt;      // per problem
    const uint32_t* recbase;
    uint32_t R;
    uint64_t* reckey;      // R x words
    uint32_t *recslot, *recfirst, *recscan;   // recfirst: 1 = the first record of its key; recscan: its exclusive scan
    int32_t *recb, *reck;  // b within the chunk
    // hash table
    uint64_t* tab;         // 0 = empty
    uint32_t *slotfirst, *slotcnt, *slotrow;
    uint64_t slotmask, seed, hashmask;
    int32_t* collide;
    // rows of the chunk
    uint32_t S;
    uint64_t* rowkey;
    int32_t *rowb, *rowk;
    uint32_t *rowcnt, *segoff, *cursor;
    const double* rowinit;
    double* rowsum;
    // segments
    uint32_t T;
    int32_t* segb;
    uint32_t* segrow;
    double *segw, *sorted;
    // scan
    const uint32_t* scan_in;
    uint32_t *scan_out, *scan_sums;
    uint32_t scan_n;
};

// ---- integer atomics: the instruction on the device, the plain operation in the CPU driver (one thread at a time)
FNN_HD uint64_t sup_cas64(uint64_t* p, uint64_t expect, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS((unsigned long long*)p, (unsigned long long)expect, (unsigned long long)v);
#else
    const uint64_t old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
FNN_HD void sup_min32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
FNN_HD uint32_t sup_add32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const uint32_t old = *p;
    *p = old + v;
    return old;
#endif
}

// ---- indices and keys
FNN_HD int64_t sup_row_start(int64_t i, int64_t n) { return i * (2 * n - i - 1) / 2; }  // k of (i, i + 1)
// k -> (i, j): an estimate from the square root, then exact integer steps
FNN_HD void sup_decode(int64_t k, int32_t n, int32_t& i, int32_t& j) {
    const double t = (double)(2 * n - 1);
    double d = t * t - 8.0 * (double)k;
    if (d < 0.0) d = 0.0;
    int64_t r = (int64_t)((t - __builtin_sqrt(d)) * 0.5);
    if (r < 0) r = 0;
    if (r > n - 2) r = n - 2;
    while (r < n - 2 && sup_row_start(r + 1, n) <= k) r++;
    while (r > 0 && sup_row_start(r, n) > k) r--;
    i = (int32_t)r;
    j = (int32_t)(r + 1 + (k - sup_row_start(r, n)));
}
FNN_HD uint64_t sup_word_mask(int32_t n, int32_t w, int32_t words) {
    return (w + 1 < words || (n & 63) == 0) ? ~0ull : ((1ull << (n & 63)) - 1ull);
}
// P: (n + 1) x words prefix sets; the split of positions i + 1 ... j, folded to the side without taxon 1
FNN_HD bool sup_key_flip(const uint64_t* P, int32_t words, int32_t i, int32_t j) {
    return ((P[(int64_t)j * words] ^ P[(int64_t)i * words]) & 1ull) != 0;
}
FNN_HD uint64_t sup_key_word(const uint64_t* P, int32_t words, int32_t n, int32_t i, int32_t j, int32_t w, bool flip) {
    const uint64_t x = P[(int64_t)j * words + w] ^ P[(int64_t)i * words + w];
    return flip ? (~x & sup_word_mask(n, w, words)) : x;
}
// word t of every prefix set from the ordering o[1 ... n] (thread t < words; an OR-scan along the positions in a register)
FNN_HD void sup_prefix_word(const int32_t* o, int32_t n, int32_t words, int32_t t, uint64_t* P) {
    uint64_t acc = 0;
    P[t] = 0;
    for (int32_t p = 1; p <= n; p++) {
        const int32_t x = o[p] - 1;
        if ((x >> 6) == t) acc |= 1ull << (x & 63);
        P[(int64_t)p * words + t] = acc;
    }
}
FNN_HD uint64_t sup_hash_end(uint64_t h) {  // (the finaliser of SplitMix64: a bijection in which every input bit reaches every output bit)
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    return h ^ (h >> 31);
}
// One word into the hash: the whole finaliser per word.  Keys are sparse (a trivial split is one bit), and a lighter step -
// one multiplication and a shift - let the top bit of one word cancel against two bits of the next under EVERY seed:
// taxa {64, 96} and {128} met in one slot in the first run on real bootstrap weights.
FNN_HD uint64_t sup_hash_step(uint64_t h, uint64_t x) { return sup_hash_end(h ^ x); }
FNN_HD bool sup_counts(const SupArgs& a, int64_t bl, int64_t k) { return a.w[bl * a.K + k] > a.thr; }

// ---- count: thread t of the workgroup of problem bl
FNN_HD void sup_count_thread(const SupArgs& a, int64_t bl, int32_t t, int32_t nt) {
    uint32_t c = 0;
    for (int64_t k = t; k < a.K; k += nt) c += sup_counts(a, bl, k) ? 1u : 0u;
    if (c) sup_add32(&a.reccnt[bl], c);
}

// ---- emit: the LDS image of one workgroup
struct SupLds {
    uint64_t* P;      // (n + 1) x words
    uint64_t* wmask;  // SUP_WAVES: the ballots of the tile
    int32_t* ord;     // n + 1
};
FNN_HD int32_t sup_lds_bytes(int32_t n, int32_t words) { return 8 * (n + 1) * words + 8 * SUP_WAVES + 4 * (n + 1); }
FNN_HD SupLds sup_lds_view(unsigned char* base, int32_t n, int32_t words) {
    SupLds L;
    L.P = (uint64_t*)base;
    L.wmask = L.P + (int64_t)(n + 1) * words;
    L.ord = (int32_t*)(L.wmask + SUP_WAVES);
    return L;
}
FNN_HD void sup_emit_load(const SupArgs& a, const SupLds& L, int64_t bl, int32_t t, int32_t nt) {
    for (int32_t p = t; p <= a.n; p += nt) L.ord[p] = a.ord[bl * (a.n + 1) + p];
}
FNN_HD void sup_emit_prefix(const SupArgs& a, const SupLds& L, int32_t t) {
    if (t < a.words) sup_prefix_word(L.ord, a.n, a.words, t, L.P);
}
// the place of thread t's record among the tile's records, from the waves' ballots; *total: the records of the tile
FNN_HD uint32_t sup_emit_place(const uint64_t* wmask, int32_t t, uint32_t* total) {
    const int32_t wave = t >> 6, lane = t & 63;
    uint32_t before = 0, tot = 0;
    for (int32_t v = 0; v < SUP_WAVES; v++) {
        const uint32_t c = (uint32_t)__builtin_popcountll(wmask[v]);
        if (v < wave) before += c;
        tot += c;
    }
    *total = tot;
    return before + (uint32_t)__builtin_popcountll(wmask[wave] & ((1ull << lane) - 1ull));
}
FNN_HD void sup_emit_record(const SupArgs& a, const uint64_t* P, int64_t bl, int64_t k, uint32_t rid) {
    if (rid >= a.R) return;  // (the weights changed between count and emit: a device array under the caller's writes)
    int32_t i, j;
    sup_decode(k, a.n, i, j);
    const bool flip = sup_key_flip(P, a.words, i, j);
    uint64_t h = a.seed;
    for (int32_t w = 0; w < a.words; w++) {
        const uint64_t x = sup_key_word(P, a.words, a.n, i, j, w, flip);
        a.reckey[(int64_t)rid * a.words + w] = x;
        h = sup_hash_step(h, x);
    }
    const uint64_t hv = (sup_hash_end(h) & a.hashmask) | SUP_USED;
    uint64_t s = sup_hash_end(hv) & a.slotmask;
    // at most half of the slots are ever taken (slots >= 2 R): an empty one is met before the walk closes
    for (uint64_t step = 0; step <= a.slotmask; step++) {
        const uint64_t old = sup_cas64(&a.tab[s], 0ull, hv);
        if (old == 0ull || old == hv) break;
        s = (s + 1) & a.slotmask;
    }
    a.recslot[rid] = (uint32_t)s;
    a.recb[rid] = (int32_t)bl;
    a.reck[rid] = (int32_t)k;
    sup_min32(&a.slotfirst[s], rid);
    if (a.b0 + bl >= a.lead) sup_add32(&a.slotcnt[s], 1u);
}

// ---- the flat kernels: one thread per item g
FNN_HD void sup_verify_thread(const SupArgs& a, uint32_t g) {
    if (g >= a.R) return;
    const uint32_t s = a.recslot[g];
    if ((uint64_t)s > a.slotmask) { *a.collide = 2; a.recfirst[g] = 0u; return; }  // (a record that emit never wrote: see sup_emit_record)
    const uint32_t f = a.slotfirst[s];
    bool same = f < a.R;
    for (int32_t w = 0; same && w < a.words; w++) same = a.reckey[(int64_t)g * a.words + w] == a.reckey[(int64_t)f * a.words + w];
    if (!same) *a.collide = 1;
    a.recfirst[g] = f == g ? 1u : 0u;
}
FNN_HD void sup_rows_thread(const SupArgs& a, uint32_t g) {
    if (g >= a.R || !a.recfirst[g]) return;
    const uint32_t row = a.recscan[g], s = a.recslot[g];
    if (row >= a.S) return;
    a.slotrow[s] = row;
    for (int32_t w = 0; w < a.words; w++) a.rowkey[(int64_t)row * a.words + w] = a.reckey[(int64_t)g * a.words + w];
    a.rowb[row] = a.recb[g];
    a.rowk[row] = a.reck[g];
    a.rowcnt[row] = a.slotcnt[s];
}
FNN_HD void sup_scatter_thread(const SupArgs& a, uint32_t g) {
    if (g >= a.R) return;
    const int64_t bl = a.recb[g];
    if (a.b0 + bl < a.lead) return;
    const uint32_t row = a.slotrow[a.recslot[g]];
    if (row >= a.S) return;
    const uint32_t pos = a.segoff[row] + sup_add32(&a.cursor[row], 1u);
    if (pos >= a.T) return;
    a.segb[pos] = (int32_t)bl;
    a.segrow[pos] = row;
    a.segw[pos] = a.w[bl * a.K + a.reck[g]];
}
FNN_HD void sup_rank_thread(const SupArgs& a, uint32_t g) {
    if (g >= a.T) return;
    const uint32_t row = a.segrow[g], off = a.segoff[row], m = a.rowcnt[row];
    const int32_t b = a.segb[g];
    uint32_t r = 0;
    for (uint32_t q = 0; q < m; q++) r += a.segb[off + q] < b ? 1u : 0u;
    a.sorted[off + r] = a.segw[g];
}
FNN_HD void sup_sum_thread(const SupArgs& a, uint32_t g) {
    if (g >= a.S) return;
    const uint32_t off = a.segoff[g], m = a.rowcnt[g];
    double s = a.rowinit[g];
    for (uint32_t q = 0; q < m; q++) s = s + a.sorted[off + q];  // the sequential sum: one rounding per addition
    a.rowsum[g] = s;
}
// exclusive scan of scan_in[0 .. scan_n): tile sums (integer atomic add), then per tile from the tile's offset
FNN_HD uint32_t sup_scan_own(const SupArgs& a, int64_t blk, int32_t t) {
    uint32_t s = 0;
    for (int32_t e = 0; e < SUP_SCAN_PER_THREAD; e++) {
        const int64_t at = blk * SUP_SCAN_TILE + (int64_t)t * SUP_SCAN_PER_THREAD + e;
        if (at < (int64_t)a.scan_n) s += a.scan_in[at];
    }
    return s;
}
FNN_HD void sup_scan_sums_thread(const SupArgs& a, int64_t blk, int32_t t) {
    const uint32_t s = sup_scan_own(a, blk, t);
    if (s) sup_add32(&a.scan_sums[blk], s);
}
FNN_HD void sup_scan_apply_thread(const SupArgs& a, int64_t blk, int32_t t, const uint32_t* part) {  // part[u]: sup_scan_own of thread u
    uint32_t pre = a.scan_sums[blk];  // (by now the exclusive prefix of the tile sums)
    for (int32_t u = 0; u < t; u++) pre += part[u];
    for (int32_t e = 0; e < SUP_SCAN_PER_THREAD; e++) {
        const int64_t at = blk * SUP_SCAN_TILE + (int64_t)t * SUP_SCAN_PER_THREAD + e;
        if (at < (int64_t)a.scan_n) { a.scan_out[at] = pre; pre += a.scan_in[at]; }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct SupTable {  // the rows in order of first appearance
    int32_t words = 0;
    std::vector<uint64_t> keys;
    std::vector<int64_t> first_b, first_k, count;
    std::vector<double> sum;
    int64_t rows() const { return (int64_t)first_b.size(); }
    int64_t append(const uint64_t* key, int64_t b, int64_t k) {
        keys.insert(keys.end(), key, key + words);
        first_b.push_back(b);
        first_k.push_back(k);
        count.push_back(0);
        sum.push_back(0.0);
        return rows() - 1;
    }
};
using SupMap = std::map<std::vector<uint64_t>, int64_t>;

inline bool sup_ordering_ok(const int32_t* o, int32_t n, std::vector<char>& seen) {
    seen.assign((size_t)n + 1, 0);
    for (int32_t p = 1; p <= n; p++) {
        if (o[p] < 1 || o[p] > n || seen[(size_t)o[p]]) return false;
        seen[(size_t)o[p]] = 1;
    }
    return true;
}
inline void sup_prefix_sets(const int32_t* o, int32_t n, int32_t words, std::vector<uint64_t>& P) {
    P.resize((size_t)(n + 1) * (size_t)words);
    for (int32_t t = 0; t < words; t++) sup_prefix_word(o, n, words, t, P.data());
}

// the host route: the definition with an ordered map; problems and, inside one, k ascending
inline int64_t sup_host_tally(int32_t n, int64_t batch, const int32_t* orderings, const double* weights, double thr, int64_t lead, SupTable& tb) {
    const int32_t words = tb.words;
    const int64_t K = (int64_t)n * (n - 1) / 2;
    SupMap rows;
    std::vector<uint64_t> P, key((size_t)words);
    int64_t records = 0;
    for (int64_t b = 0; b < batch; b++) {
        const double* w = weights + b * K;
        bool built = false;
        int64_t k = 0;
        for (int32_t i = 0; i < n - 1; i++)
            for (int32_t j = i + 1; j < n; j++, k++) {
                if (!(w[k] > thr)) continue;
                if (!built) { sup_prefix_sets(orderings + b * (n + 1), n, words, P); built = true; }
                records++;
                const bool flip = sup_key_flip(P.data(), words, i, j);
                for (int32_t q = 0; q < words; q++) key[(size_t)q] = sup_key_word(P.data(), words, n, i, j, q, flip);
                auto it = rows.find(key);
                int64_t row;
                if (it == rows.end()) { row = tb.append(key.data(), b, k); rows.emplace(key, row); }
                else row = it->second;
                if (b >= lead) { tb.count[(size_t)row]++; tb.sum[(size_t)row] = tb.sum[(size_t)row] + w[k]; }
            }
    }
    return records;
}

inline int32_t sup_split_keys(const char* who, int32_t n, const int32_t* ordering, const int64_t* k, int64_t count, uint64_t* keys_out) {
    const std::string W = std::string(who) + ": ";
    if (n < 2 || count < 0) return fail(FNN_EINVAL, W + "needs n >= 2 and count >= 0");
    if (count == 0) return FNN_OK;
    if (!ordering || !k || !keys_out) return fail(FNN_EINVAL, W + "NULL argument");
    std::vector<char> seen;
    if (!sup_ordering_ok(ordering, n, seen)) return fail(FNN_EINVAL, W + "ordering is not a permutation of 1..n");
    const int64_t K = (int64_t)n * (n - 1) / 2;
    for (int64_t q = 0; q < count; q++)
        if (k[q] < 0 || k[q] >= K) return fail(FNN_EINVAL, W + "split index " + std::to_string(k[q]) + " is outside 0 ... n(n-1)/2 - 1");
    const int32_t words = (n + 63) / 64;
    std::vector<uint64_t> P;
    sup_prefix_sets(ordering, n, words, P);
    for (int64_t q = 0; q < count; q++) {
        int32_t i, j;
        sup_decode(k[q], n, i, j);
        const bool flip = sup_key_flip(P.data(), words, i, j);
        for (int32_t w = 0; w < words; w++) keys_out[q * words + w] = sup_key_word(P.data(), words, n, i, j, w, flip);
    }
    return FNN_OK;
}

inline int sup_route_switch() {  // FNN_SUPPORT_ROUTE=kernel|host: 0 / 1; -1: not set
    const char* e = std::getenv("FNN_SUPPORT_ROUTE");
    if (e && !std::strcmp(e, "kernel")) return FNN_SUPPORT_ROUTE_KERNEL;
    if (e && !std::strcmp(e, "host")) return FNN_SUPPORT_ROUTE_HOST;
    return -1;
}
inline uint64_t sup_hash_mask() {  // FNN_SUPPORT_HASH_BITS=<1..64>
    if (const char* e = std::getenv("FNN_SUPPORT_HASH_BITS")) {
        const int v = std::atoi(e);
        if (v >= 1 && v < 64) return (1ull << v) - 1ull;
    }
    return ~0ull;
}

// exclusive scan of in[0 .. N) into out on the device; *total: the sum.  sums: a buffer of ceil(N / SUP_SCAN_TILE) words
template <class B>
int32_t sup_scan(B& be, SupArgs a, const uint32_t* in, uint32_t N, uint32_t* out, uint32_t* sums, std::vector<uint32_t>& hs, uint32_t* total,
                 double* t_kernel_s) {
    const int64_t tiles = ((int64_t)N + SUP_SCAN_TILE - 1) / SUP_SCAN_TILE;
    *total = 0;
    if (N == 0) return FNN_OK;
    a.scan_in = in; a.scan_out = out; a.scan_sums = sums; a.scan_n = N;
    double tk = 0.0;
    if (be.fill(sums, 0, sizeof(uint32_t) * (size_t)tiles) != FNN_OK || be.run(SUP_K_SCAN_SUMS, a, tiles, &tk) != FNN_OK) return FNN_EHIP;
    *t_kernel_s += tk;
    hs.resize((size_t)tiles);
    if (be.d2h(hs.data(), sums, sizeof(uint32_t) * (size_t)tiles) != FNN_OK) return FNN_EHIP;
    uint64_t run = 0;
    for (int64_t t = 0; t < tiles; t++) { const uint32_t s = hs[(size_t)t]; hs[(size_t)t] = (uint32_t)run; run += s; }
    if (run >> 32) { be.last = "scan total does not fit 32 bits"; return FNN_EHIP; }
    *total = (uint32_t)run;
    if (be.h2d(sums, hs.data(), sizeof(uint32_t) * (size_t)tiles) != FNN_OK || be.run(SUP_K_SCAN_APPLY, a, tiles, &tk) != FNN_OK) return FNN_EHIP;
    *t_kernel_s += tk;
    return FNN_OK;
}

// fnn_split_support[_device]_f64 over a backend B (HIP: fnn_support.hip; CPU driver: tests/emu):
//   open(device); alloc / release; fill(ptr, byte, bytes); h2d / d2h; run(kernel, args, items, &t_kernel_s); err(); last
// (items: problems for SUP_K_COUNT / SUP_K_EMIT, tiles for the scans, threads' items for the flat kernels)
template <class B>
int32_t support_call(B& be, const char* who, int32_t n, int64_t batch, const int32_t* orderings, const double* weights, bool on_device, double thr,
                     int64_t lead, int32_t device, uint64_t* keys_out, int64_t* first_b_out, int64_t* first_k_out, int64_t* counts_out,
                     double* weight_sum_out, int64_t capacity, int64_t* count_out, fnn_support_stats* stats) {
    const double t0 = now_s();
    const std::string W = std::string(who) + ": ";
    fnn_support_stats st{};
    if (n < 2 || batch < 0 || capacity < 0) return fail(FNN_EINVAL, W + "needs n >= 2, batch >= 0 and capacity >= 0");
    if (n > SUP_MAX_N) return fail(FNN_EINVAL, W + "n = " + std::to_string(n) + " is above fnn_split_support_max_n() = " + std::to_string(SUP_MAX_N));
    if (lead < 0 || lead > batch) return fail(FNN_EINVAL, W + "needs 0 <= lead <= batch");
    if (thr != thr) return fail(FNN_EINVAL, W + "the threshold is a NaN");
    if (!count_out) return fail(FNN_EINVAL, W + "NULL argument");
    if (capacity > 0 && (!keys_out || !first_b_out || !first_k_out || !counts_out || !weight_sum_out)) return fail(FNN_EINVAL, W + "NULL argument");
    const int32_t words = (n + 63) / 64;
    st.words = words;
    st.route = FNN_SUPPORT_ROUTE_HOST;
    if (batch == 0) { *count_out = 0; st.t_total_s = now_s() - t0; if (stats) *stats = st; return FNN_OK; }
    if (!orderings || !weights) return fail(FNN_EINVAL, W + "NULL argument");
    {
        std::vector<char> seen;
        for (int64_t b = 0; b < batch; b++)
            if (!sup_ordering_ok(orderings + b * (n + 1), n, seen))
                return fail(FNN_EINVAL, W + "problem " + std::to_string(b) + ": ordering is not a permutation of 1..n");
    }
    st.n_problems = batch;
    const int64_t K = (int64_t)n * (n - 1) / 2;
    SupTable tb;
    tb.words = words;
    const int sw = sup_route_switch();
    bool kernel = sw >= 0 ? sw == FNN_SUPPORT_ROUTE_KERNEL : batch * n * n >= SUP_MIN_WORK;
    bool opened = false;

    if (kernel) {
        const int32_t rc = be.open(device);
        if (rc != FNN_OK) return fail(rc, W + be.err());
        opened = true;
        const uint64_t hashmask = sup_hash_mask();
        int64_t chunk = batch_chunk(batch, 8 * K, false);
        if (chunk > (((int64_t)1 << 31) - 1) / K) chunk = (((int64_t)1 << 31) - 1) / K;  // (record ids are 32-bit; K <= 523 776)
        int32_t* d_ord = (int32_t*)be.alloc(sizeof(int32_t) * (size_t)chunk * (size_t)(n + 1));
        double* d_w = on_device ? nullptr : (double*)be.alloc(sizeof(double) * (size_t)chunk * (size_t)K);
        uint32_t* d_reccnt = (uint32_t*)be.alloc(sizeof(uint32_t) * (size_t)chunk);
        uint32_t* d_recbase = (uint32_t*)be.alloc(sizeof(uint32_t) * (size_t)chunk);
        int32_t* d_collide = (int32_t*)be.alloc(sizeof(int32_t));
        if (!d_ord || (!on_device && !d_w) || !d_reccnt || !d_recbase || !d_collide) return fail(FNN_ENOMEM, W + "device allocation failed");
        std::vector<uint32_t> hcnt, hs, hrowcnt;
        std::vector<uint64_t> hkey;
        std::vector<int32_t> hrowb, hrowk;
        std::vector<double> hinit, hsum;
        std::vector<int64_t> grow;
        SupMap rows;
        bool mapped = false;
        for (int64_t b0 = 0; b0 < batch && kernel; b0 += chunk) {
            const int64_t cnt = batch - b0 < chunk ? batch - b0 : chunk;
            st.chunks++;
            const double tu = now_s();
            if (be.h2d(d_ord, orderings + b0 * (n + 1), sizeof(int32_t) * (size_t)cnt * (size_t)(n + 1)) != FNN_OK ||
                (!on_device && be.h2d(d_w, weights + b0 * K, sizeof(double) * (size_t)cnt * (size_t)K) != FNN_OK) ||
                be.fill(d_reccnt, 0, sizeof(uint32_t) * (size_t)cnt) != FNN_OK)
                return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")");
            st.t_upload_s += now_s() - tu;
            SupArgs a{};
            a.ord = d_ord; a.w = on_device ? weights + b0 * K : d_w; a.n = n; a.words = words; a.K = K; a.cnt = cnt; a.b0 = b0; a.lead = lead;
            a.thr = thr; a.reccnt = d_reccnt; a.recbase = d_recbase; a.collide = d_collide; a.hashmask = hashmask;
            double tk = 0.0;
            if (be.run(SUP_K_COUNT, a, cnt, &tk) != FNN_OK) return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")");
            st.t_kernel_s += tk;
            hcnt.resize((size_t)cnt);
            if (be.d2h(hcnt.data(), d_reccnt, sizeof(uint32_t) * (size_t)cnt) != FNN_OK) return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
            uint64_t R64 = 0;
            for (int64_t b = 0; b < cnt; b++) { const uint32_t c = hcnt[(size_t)b]; hcnt[(size_t)b] = (uint32_t)R64; R64 += c; }
            const uint32_t R = (uint32_t)R64;
            st.n_records += (int64_t)R;
            if (R == 0) continue;
            uint64_t slots = 64;
            while (slots < 2 * R64) slots <<= 1;
            if ((int64_t)slots > st.table_slots) st.table_slots = (int64_t)slots;
            const int64_t tiles = ((int64_t)R + SUP_SCAN_TILE - 1) / SUP_SCAN_TILE;
            // the chunk's record and table buffers (released at the end of the chunk)
            std::vector<void*> mine;
            auto take = [&](size_t bytes) { void* p = be.alloc(bytes); if (p) mine.push_back(p); return p; };
            auto drop = [&] { for (void* p : mine) be.release(p); mine.clear(); };
            a.R = R;
            a.reckey = (uint64_t*)take(8 * (size_t)R * (size_t)words);
            a.recslot = (uint32_t*)take(4 * (size_t)R);
            a.recfirst = (uint32_t*)take(4 * (size_t)R);
            a.recscan = (uint32_t*)take(4 * (size_t)R);
            a.recb = (int32_t*)take(4 * (size_t)R);
            a.reck = (int32_t*)take(4 * (size_t)R);
            a.tab = (uint64_t*)take(8 * (size_t)slots);
            a.slotfirst = (uint32_t*)take(4 * (size_t)slots);
            a.slotcnt = (uint32_t*)take(4 * (size_t)slots);
            a.slotrow = (uint32_t*)take(4 * (size_t)slots);
            uint32_t* d_sums = (uint32_t*)take(4 * (size_t)tiles);
            if (mine.size() != 11) { drop(); return fail(FNN_ENOMEM, W + "device allocation failed"); }
            a.slotmask = slots - 1;
            if (be.h2d(d_recbase, hcnt.data(), sizeof(uint32_t) * (size_t)cnt) != FNN_OK) { drop(); return fail(FNN_EHIP, W + "upload failed (" + be.err() + ")"); }
            int32_t flag = 1;
            for (int32_t attempt = 0; flag && attempt <= SUP_RETRIES; attempt++) {
                if (attempt) st.hash_retries++;
                a.seed = splitmix64_at(SUP_SEED, (uint64_t)st.hash_retries);
                if (be.fill(a.recslot, 0xFF, 4 * (size_t)R) != FNN_OK || be.fill(a.tab, 0, 8 * (size_t)slots) != FNN_OK || be.fill(a.slotfirst, 0xFF, 4 * (size_t)slots) != FNN_OK ||
                    be.fill(a.slotcnt, 0, 4 * (size_t)slots) != FNN_OK || be.fill(a.slotrow, 0xFF, 4 * (size_t)slots) != FNN_OK ||
                    be.fill(d_collide, 0, sizeof(int32_t)) != FNN_OK || be.run(SUP_K_EMIT, a, cnt, &tk) != FNN_OK)
                    { drop(); return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")"); }
                st.t_kernel_s += tk;
                if (be.run(SUP_K_VERIFY, a, (int64_t)R, &tk) != FNN_OK || be.d2h(&flag, d_collide, sizeof(int32_t)) != FNN_OK)
                    { drop(); return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")"); }
                st.t_kernel_s += tk;
                if (flag) st.reserved[0] = flag;  // why the last repeat was needed: 1 two keys with one hash, 2 a record that emit never wrote
            }
            if (flag) { drop(); kernel = false; break; }  // two keys with one hash under every seed tried: the host route
            uint32_t S = 0;
            if (sup_scan(be, a, a.recfirst, R, a.recscan, d_sums, hs, &S, &st.t_kernel_s) != FNN_OK) { drop(); return fail(FNN_EHIP, W + "scan failed (" + be.err() + ")"); }
            a.S = S;
            a.rowkey = (uint64_t*)take(8 * (size_t)S * (size_t)words);
            a.rowb = (int32_t*)take(4 * (size_t)S);
            a.rowk = (int32_t*)take(4 * (size_t)S);
            a.rowcnt = (uint32_t*)take(4 * (size_t)S);
            a.segoff = (uint32_t*)take(4 * (size_t)S);
            a.cursor = (uint32_t*)take(4 * (size_t)S);
            double* d_init = (double*)take(8 * (size_t)S);
            a.rowsum = (double*)take(8 * (size_t)S);
            if (mine.size() != 19) { drop(); return fail(FNN_ENOMEM, W + "device allocation failed"); }
            a.rowinit = d_init;
            if (be.run(SUP_K_ROWS, a, (int64_t)R, &tk) != FNN_OK) { drop(); return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")"); }
            st.t_kernel_s += tk;
            hkey.resize((size_t)S * (size_t)words); hrowb.resize(S); hrowk.resize(S); hrowcnt.resize(S); hinit.assign(S, 0.0); hsum.resize(S); grow.resize(S);
            if (be.d2h(hkey.data(), a.rowkey, 8 * (size_t)S * (size_t)words) != FNN_OK || be.d2h(hrowb.data(), a.rowb, 4 * (size_t)S) != FNN_OK ||
                be.d2h(hrowk.data(), a.rowk, 4 * (size_t)S) != FNN_OK || be.d2h(hrowcnt.data(), a.rowcnt, 4 * (size_t)S) != FNN_OK)
                { drop(); return fail(FNN_EHIP, W + "download failed (" + be.err() + ")"); }
            // the chunk's rows meet the table: a key of an earlier chunk keeps its row and hands over its partial sum
            if (tb.rows() == 0) {
                for (uint32_t l = 0; l < S; l++) grow[l] = tb.append(&hkey[(size_t)l * (size_t)words], b0 + hrowb[l], hrowk[l]);
            } else {
                if (!mapped) {
                    for (int64_t r = 0; r < tb.rows(); r++)
                        rows.emplace(std::vector<uint64_t>(tb.keys.begin() + r * words, tb.keys.begin() + (r + 1) * words), r);
                    mapped = true;
                }
                for (uint32_t l = 0; l < S; l++) {
                    std::vector<uint64_t> key(hkey.begin() + (size_t)l * (size_t)words, hkey.begin() + ((size_t)l + 1) * (size_t)words);
                    auto it = rows.find(key);
                    if (it == rows.end()) { grow[l] = tb.append(key.data(), b0 + hrowb[l], hrowk[l]); rows.emplace(std::move(key), grow[l]); }
                    else { grow[l] = it->second; hinit[l] = tb.sum[(size_t)it->second]; }
                }
            }
            uint32_t T = 0;
            if (be.h2d(d_init, hinit.data(), 8 * (size_t)S) != FNN_OK || be.fill(a.cursor, 0, 4 * (size_t)S) != FNN_OK ||
                sup_scan(be, a, a.rowcnt, S, a.segoff, d_sums, hs, &T, &st.t_kernel_s) != FNN_OK)
                { drop(); return fail(FNN_EHIP, W + "scan failed (" + be.err() + ")"); }
            a.T = T;
            a.segb = (int32_t*)take(4 * (size_t)T);
            a.segrow = (uint32_t*)take(4 * (size_t)T);
            a.segw = (double*)take(8 * (size_t)T);
            a.sorted = (double*)take(8 * (size_t)T);
            if (mine.size() != 23) { drop(); return fail(FNN_ENOMEM, W + "device allocation failed"); }
            if (T) {
                if (be.run(SUP_K_SCATTER, a, (int64_t)R, &tk) != FNN_OK) { drop(); return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")"); }
                st.t_kernel_s += tk;
                if (be.run(SUP_K_RANK, a, (int64_t)T, &tk) != FNN_OK) { drop(); return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")"); }
                st.t_kernel_s += tk;
            }
            if (be.run(SUP_K_SUM, a, (int64_t)S, &tk) != FNN_OK || be.d2h(hsum.data(), a.rowsum, 8 * (size_t)S) != FNN_OK)
                { drop(); return fail(FNN_EHIP, W + "kernel failed (" + be.err() + ")"); }
            st.t_kernel_s += tk;
            for (uint32_t l = 0; l < S; l++) {
                tb.count[(size_t)grow[l]] += (int64_t)hrowcnt[l];
                tb.sum[(size_t)grow[l]] = hsum[l];
            }
            drop();
        }
    }
    if (kernel) st.route = FNN_SUPPORT_ROUTE_KERNEL;
    else {
        // the host route: below the crossover, by the switch, or after the repeats ran out (the table starts again)
        std::vector<double> hw;
        const double* w = weights;
        if (on_device) {
            if (!opened) { const int32_t rc = be.open(device); if (rc != FNN_OK) return fail(rc, W + be.err()); }
            hw.resize((size_t)batch * (size_t)K);
            const double tu = now_s();
            if (be.d2h(hw.data(), weights, sizeof(double) * hw.size()) != FNN_OK) return fail(FNN_EHIP, W + "download failed (" + be.err() + ")");
            st.t_upload_s += now_s() - tu;
            w = hw.data();
        }
        tb = SupTable();
        tb.words = words;
        st.route = FNN_SUPPORT_ROUTE_HOST;
        st.n_records = sup_host_tally(n, batch, orderings, w, thr, lead, tb);
    }
    const int64_t S = tb.rows(), fillrows = S < capacity ? S : capacity;
    st.n_splits = S;
    if (fillrows > 0) {
        std::memcpy(keys_out, tb.keys.data(), 8 * (size_t)fillrows * (size_t)words);
        std::memcpy(first_b_out, tb.first_b.data(), 8 * (size_t)fillrows);
        std::memcpy(first_k_out, tb.first_k.data(), 8 * (size_t)fillrows);
        std::memcpy(counts_out, tb.count.data(), 8 * (size_t)fillrows);
        std::memcpy(weight_sum_out, tb.sum.data(), 8 * (size_t)fillrows);
    }
    *count_out = S;
    st.t_total_s = now_s() - t0;
    if (stats) *stats = st;
    return FNN_OK;
}

}  // namespace fnn
#endif
