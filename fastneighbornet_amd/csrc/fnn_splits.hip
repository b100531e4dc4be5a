// fnn_splits.hip -- circular split weights (non-negative least squares) on gfx950.
//
// The "next" row N1 of SURVEY.md 8(f): given the circular ordering, the weights of the n(n-1)/2 circular splits are
// the solution of the non-negative least-squares problem min |A x - d|, x >= 0 - what the reference's live path computes
// with a dense design matrix and a third-party Lawson-Hanson solver (FastNN.java:401-454), here on the implicit
// operators of CircularSplitWeights.java (:603-731 calculateAtx / calculateAb) with the re-ordering of the distances by
// the circular ordering restored (setupD :202-211) and the result in the index space of the live path
// (FastNN.java:405-419).  Method: the closed-form unconstrained optimum if it is feasible; else Lawson-Hanson "from
// below" on closed-form entries of A^T A with an explicitly maintained inverse of the free block (rank-one updates by
// rocBLAS, rebuilds by rocSOLVER), Kuhn-Tucker test on a fresh inverse; the reference's own active-set / conjugate-
// gradient method (:366-557 runActiveConjugate, :769-831 circularConjugateGrads, :283-337 worstIndices) remains as the
// fallback and behind FNN_SW_REFERENCE_METHOD=1 (it stops short of the optimum by ~1e-5: DESIGN.md section 7).
//
// GPU formulation.  All vectors of the method (split weights x, distances d, residuals ...) are
// kept as the strict upper triangle of dense n x n fp64 arrays: entry [i][j], i < j, is the split
// (i, j) = cycle positions {i+1 .. j}, or the pair of positions (i, j).  The reference evaluates
// A b and A^T y with anti-diagonal recurrences (n - 1 dependent sweeps); here both are O(1)
// gathers from a 2-D inclusive prefix sum P of the argument (row scan, LDS-tiled transpose, row
// scan; P is held transposed):
//   (A b)[a][b]   = sum of x over the splits that separate positions a < b
//                 = rect(i in [0,a-1], j in [a,b-1]) + rect(i in [a,b-1], j in [b,n-1])
//   (A^T y)[i][j] = sum of y over the pairs separated by split (i,j), S = {i+1..j}
//                 = (RS[j] - RS[i]) - 2 (P[j][j] - P[i][j]),  RS = prefix of the row sums of the
//                   symmetric completion of y.
// Everything is bandwidth-bound elementwise / scan work on n^2 doubles; the control flow of the
// solver (a handful of scalars per step) runs on the host.  The optimum is unique (A is square and non-singular); the
// tests hold the weights to 1e-6 of a dense NNLS solve of the live path's problem where that is computable (n <= 64),
// to the known weights of generated circular metrics up to 4096 taxa, and to the Kuhn-Tucker conditions beyond.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "fnn_engine.h"  // fnn::fail / the thread-local error message shared with fnn_hip.hip
#include "fnn_splits_plan.h"  // the switches, the capacity plan and the block method's pure host steps

namespace fnnsw {

constexpr double CG_EPSILON = 1e-8;  // CircularSplitWeights.java:54
constexpr int T = 256;

#define SWOK(x) ((x) == hipSuccess)

// ---------------------------------------------------------------- 2-D prefix sum
// row scan in place: one workgroup per row
// Scalars of the conjugate-gradient loop live on the device (one host read per CG_CHECK iterations);
// every kernel of an iteration returns at once when the loop has ended (sc[SC_DONE]).
enum { SC_RHO = 0, SC_RHO_OLD, SC_PW, SC_TOL2, SC_DONE, SC_K, SC_ALPHA, SC_BETA, SC_KMAX, SC_WORDS = 16 };
#define CG_SKIP(sc) do { if ((sc) != nullptr && (sc)[SC_DONE] != 0.0) return; } while (0)

// row scan: dst row = inclusive prefix of src row; one workgroup per row
__global__ __launch_bounds__(T) void k_rowscan(const double* src, double* a, int n, int64_t ld, const double* sc) {
    __shared__ double wsum[T / 64];
    __shared__ double carry_s;
    CG_SKIP(sc);
    const double* srow = src + (int64_t)blockIdx.x * ld;
    double* row = a + (int64_t)blockIdx.x * ld;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0.0;
    __syncthreads();
    for (int base = 0; base < n; base += T) {
        const int i = base + (int)threadIdx.x;
        double v = i < n ? srow[i] : 0.0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double t = __shfl_up(v, d, 64);
            if (lane >= d) v += t;
        }
        if (lane == 63) wsum[w] = v;
        __syncthreads();
        double pre = carry_s;
        for (int k = 0; k < w; k++) pre += wsum[k];
        v += pre;
        if (i < n) row[i] = v;
        __syncthreads();
        if (threadIdx.x == T - 1) carry_s = v;
        __syncthreads();
    }
}

// out = in^T (n x n), 32 x 32 tiles through LDS
__global__ __launch_bounds__(T) void k_transpose(const double* in, double* out, int n, int64_t ld, const double* sc) {
    __shared__ double tile[32][33];
    CG_SKIP(sc);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8) {
        const int r = by + k, c = bx + tx;
        tile[k][tx] = (r < n && c < n) ? in[(int64_t)r * ld + c] : 0.0;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int r = bx + k, c = by + tx;
        if (r < n && c < n) out[(int64_t)r * ld + c] = tile[tx][k];
    }
}

// ---------------------------------------------------------------- operators (gathers from the transposed prefix Pt[j][i] = P[i][j])
__device__ __forceinline__ double PT(const double* Pt, int64_t ld, int i, int j) {  // P[i][j], -1 -> 0
    return (i < 0 || j < 0) ? 0.0 : Pt[(int64_t)j * ld + i];
}

// d[a][b] = (A x)[a][b] for a < b, from the prefix of x
__global__ __launch_bounds__(T) void k_ab(const double* Pt, double* d, int n, int64_t ld, const double* sc) {
    CG_SKIP(sc);
    const int b = blockIdx.x * T + threadIdx.x, a = blockIdx.y;
    if (b >= n || a >= b) return;
    const double first = PT(Pt, ld, a - 1, b - 1) - PT(Pt, ld, a - 1, a - 1);
    const double second = (PT(Pt, ld, b - 1, n - 1) - PT(Pt, ld, a - 1, n - 1)) - (PT(Pt, ld, b - 1, b - 1) - PT(Pt, ld, a - 1, b - 1));
    d[(int64_t)a * ld + b] = first + second;
}

// RS = inclusive prefix of the row sums of the symmetric completion (one workgroup)
__global__ __launch_bounds__(1024) void k_scan1(const double* Qt, double* v, int n, int64_t ld, const double* sc) {
    __shared__ double wsum[16];
    __shared__ double carry_s;
    CG_SKIP(sc);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0.0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int i = base + (int)threadIdx.x;
        double x = 0.0;
        if (i < n) x = (PT(Qt, ld, i, n - 1) - PT(Qt, ld, i - 1, n - 1)) + (PT(Qt, ld, n - 1, i) - PT(Qt, ld, n - 1, i - 1));
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double t = __shfl_up(x, d, 64);
            if (lane >= d) x += t;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        double pre = carry_s;
        for (int k = 0; k < w; k++) pre += wsum[k];
        x += pre;
        if (i < n) v[i] = x;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = x;
        __syncthreads();
    }
}
// p[i][j] = (A^T y)[i][j] for i < j
// (mask: entries of the active set are written as 0, circularConjugateGrads :817-819)
__global__ __launch_bounds__(T) void k_atx(const double* Qt, const double* RS, double* p, int n, int64_t ld, const uint8_t* mask,
                                           const double* sc) {
    CG_SKIP(sc);
    const int j = blockIdx.x * T + threadIdx.x, i = blockIdx.y;
    if (j >= n || i >= j) return;
    const double inside = PT(Qt, ld, j, j) - PT(Qt, ld, i, j);
    const int64_t k = (int64_t)i * ld + j;
    p[k] = (mask != nullptr && mask[k]) ? 0.0 : (RS[j] - RS[i]) - 2.0 * inside;
}

// ---------------------------------------------------------------- setup kernels
// d'[a][b] = D[ord[a+1]-1][ord[b+1]-1] for a < b, 0 elsewhere (restored setupD)
__global__ __launch_bounds__(T) void k_reorder(const double* D, int64_t ldD, const int32_t* ord, double* d, int n, int64_t ld) {
    const int b = blockIdx.x * T + threadIdx.x, a = blockIdx.y;
    if (b >= n) return;
    double v = 0.0;
    if (a < b) v = D[(int64_t)(ord[a + 1] - 1) * ldD + (ord[b + 1] - 1)];
    d[(int64_t)a * ld + b] = v;
}
// Chepoi & Fichet closed form of the unconstrained optimum (runUnconstrainedLS :247-271), with dd(a,b)
// the re-ordered distance of positions a, b (either order, 0 on the diagonal):
//   x[i][j] = ( dd(i,j) + dd(i+1,j+1) - dd(i,j+1) - dd(i+1,j) ) / 2, positions taken modulo n
__device__ __forceinline__ double dd(const double* d, int64_t ld, int a, int b) {
    if (a == b) return 0.0;
    return a < b ? d[(int64_t)a * ld + b] : d[(int64_t)b * ld + a];
}
__global__ __launch_bounds__(T) void k_unconstrained(const double* d, double* x, int n, int64_t ld) {
    const int j = blockIdx.x * T + threadIdx.x, i = blockIdx.y;
    if (j >= n) return;
    double v = 0.0;
    if (i < j) {
        const int i1 = i + 1, j1 = (j + 1) % n;
        v = (dd(d, ld, i, j) + dd(d, ld, i1, j1) - dd(d, ld, i, j1) - dd(d, ld, i1, j)) / 2.0;
    }
    x[(int64_t)i * ld + j] = v;
}

// ---------------------------------------------------------------- vector kernels over the strict upper triangle
enum { OP_COPY = 0, OP_R_INIT, OP_P_UPDATE, OP_W_MASK, OP_XR_UPDATE, OP_CONTRACT, OP_MOVE_OLD, OP_GRAD };
struct VecArgs {
    double* a; double* b; const double* c; const double* e; uint8_t* act;
    double s0, s1;
    int n; int64_t ld;
    const double* sc;  // device scalars of the CG loop (nullptr: s0 / s1 are the arguments)
};
template <int OP>
__global__ __launch_bounds__(T) void k_vec(VecArgs g) {
    CG_SKIP(g.sc);
    const int j = blockIdx.x * T + threadIdx.x, i = blockIdx.y;
    if (j >= g.n || i >= j) return;
    const int64_t k = (int64_t)i * g.ld + j;
    if (OP == OP_COPY) g.a[k] = g.c[k];
    else if (OP == OP_R_INIT) g.a[k] = g.act[k] ? 0.0 : g.c[k] - g.a[k];            // r = active ? 0 : b - r   (:785-789)
    else if (OP == OP_P_UPDATE) g.a[k] = (g.sc[SC_K] == 0.0) ? g.c[k] : g.c[k] + g.sc[SC_BETA] * g.a[k];  // p = r (k = 1) | r + beta p (:801-808)
    else if (OP == OP_W_MASK) { if (g.act[k]) g.a[k] = 0.0; }                         // w = 0 on the active set  (:817-819)
    else if (OP == OP_XR_UPDATE) { const double al = g.sc[SC_ALPHA]; g.a[k] += al * g.c[k]; g.b[k] -= al * g.e[k]; }  // x += alpha p; r -= alpha w (:826-829)
    else if (OP == OP_CONTRACT) {                                                     // worstIndices + contraction (:411-430)
        const double v = g.a[k];
        if (v < g.s0 || (g.s1 != 0.0 && v == g.s0)) { g.a[k] = 0.0; g.act[k] = 1; }
    } else if (OP == OP_MOVE_OLD) { if (!g.act[k]) g.b[k] += g.s0 * (g.a[k] - g.b[k]); }  // old_x += min_xi (x - old_x) (:452-454)
    else if (OP == OP_GRAD) g.a[k] = (g.a[k] - g.c[k]) * 2.0;                          // r = 2 (AtWAx - AtWd)     (:478-479)
}

// reductions: per-workgroup partials, folded by a second launch (fixed order: reproducible)
struct Best { double v; int64_t k; };
enum { RD_DOT = 0, RD_COUNT_NEG, RD_COUNT_LT, RD_COUNT_EQ, RD_MIN_RATIO, RD_MIN_ACTIVE_GRAD, RD_ANY_NEG, RD_MAX_UNMASKED, RD_COUNT_NONFINITE };
template <int RD>
__global__ __launch_bounds__(T) void k_reduce(const double* a, const double* b, const uint8_t* act, double s0, int n, int64_t ld,
                                              double* partial, Best* bpartial, const double* sc) {
    __shared__ double sh[T / 64];
    __shared__ Best shb[T / 64];
    CG_SKIP(sc);
    double acc = 0.0;
    Best best{INFINITY, INT64_MAX};
    for (int i = blockIdx.y; i < n; i += gridDim.y)
        for (int j = blockIdx.x * T + threadIdx.x; j < n; j += gridDim.x * T) {
            if (i >= j) continue;
            const int64_t k = (int64_t)i * ld + j;
            if (RD == RD_DOT) acc += a[k] * b[k];
            else if (RD == RD_COUNT_NEG) acc += a[k] < 0.0 ? 1.0 : 0.0;
            else if (RD == RD_COUNT_LT) acc += (a[k] < 0.0 && a[k] < s0) ? 1.0 : 0.0;
            else if (RD == RD_COUNT_EQ) acc += (a[k] < 0.0 && a[k] == s0) ? 1.0 : 0.0;
            else if (RD == RD_COUNT_NONFINITE) acc += (fabs(a[k]) <= DBL_MAX) ? 0.0 : 1.0;  // (NaN compares false)
            else if (RD == RD_MIN_RATIO) {  // first minimum of old_x / (old_x - x) over x < 0 (:434-445)
                if (a[k] < 0.0) {
                    const double xi = b[k] / (b[k] - a[k]);
                    if (xi < best.v || (xi == best.v && k < best.k)) { best.v = xi; best.k = k; }
                }
            } else if (RD == RD_MAX_UNMASKED) {  // first maximum of a over the entries outside the mask (as the minimum of -a)
                if (!act[k]) {
                    const double gv = -a[k];
                    if (gv < best.v || (gv == best.v && k < best.k)) { best.v = gv; best.k = k; }
                }
            } else if (RD == RD_MIN_ACTIVE_GRAD) {  // first minimum of the gradient over the active set (:480-487)
                if (act[k]) {
                    const double gv = a[k];
                    if (gv < best.v || (gv == best.v && k < best.k)) { best.v = gv; best.k = k; }
                }
            }
        }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (RD == RD_MIN_RATIO || RD == RD_MIN_ACTIVE_GRAD || RD == RD_MAX_UNMASKED) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            Best o;
            o.v = __shfl_down(best.v, off, 64);
            o.k = __shfl_down((long long)best.k, off, 64);
            if (o.v < best.v || (o.v == best.v && o.k < best.k)) best = o;
        }
        if (lane == 0) shb[w] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < T / 64; q++)
                if (shb[q].v < best.v || (shb[q].v == best.v && shb[q].k < best.k)) best = shb[q];
            bpartial[blockIdx.y * gridDim.x + blockIdx.x] = best;
        }
    } else {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) sh[w] = acc;
        __syncthreads();
        if (threadIdx.x == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    }
}
// the scalars of one CG step from the partial sums of the preceding k_reduce<RD_DOT> (one workgroup;
// fixed summation order).  stage 0: rho of the start residual; 1: alpha = rho / p.w; 2: the new rho,
// beta, the iteration count and the loop condition  rho > e_0^2 && k < kmax  (:795)
__global__ __launch_bounds__(T) void k_cg_scalar(const double* partial, int np, double* sc, int stage) {
    __shared__ double sh[T / 64];
    if (stage != 0 && sc[SC_DONE] != 0.0) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += T) acc += partial[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double sum = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    if (stage == 0) {
        sc[SC_RHO] = sum; sc[SC_RHO_OLD] = 0.0; sc[SC_K] = 0.0;
        sc[SC_DONE] = (sum > sc[SC_TOL2] && 0.0 < sc[SC_KMAX]) ? 0.0 : 1.0;
    } else if (stage == 1) {
        sc[SC_PW] = sum;
        sc[SC_ALPHA] = sc[SC_RHO] / sum;
    } else {
        const double rho_old = sc[SC_RHO];
        sc[SC_RHO_OLD] = rho_old;
        sc[SC_RHO] = sum;
        sc[SC_BETA] = sum / rho_old;
        const double k = sc[SC_K] + 1.0;
        sc[SC_K] = k;
        sc[SC_DONE] = (sum > sc[SC_TOL2] && k < sc[SC_KMAX]) ? 0.0 : 1.0;
    }
}
// extreme negative values for the bisection of the cutoff
__global__ __launch_bounds__(T) void k_minneg(const double* a, int n, int64_t ld, double* partial) {
    __shared__ double sh[T / 64];
    double mn = 0.0;
    for (int i = blockIdx.y; i < n; i += gridDim.y)
        for (int j = blockIdx.x * T + threadIdx.x; j < n; j += gridDim.x * T)
            if (i < j) { const double v = a[(int64_t)i * ld + j]; if (v < mn) mn = v; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const double o = __shfl_down(mn, off, 64); if (o < mn) mn = o; }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mn;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < T / 64; q++) if (sh[q] < mn) mn = sh[q];
        partial[blockIdx.y * gridDim.x + blockIdx.x] = mn;
    }
}
__global__ __launch_bounds__(T) void k_fill(double* a, int64_t count, double v) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    if (i < count) a[i] = v;
}
// live[k] over (i, j), 0 <= i < j <= n-1, from the fast algorithm's x
__global__ __launch_bounds__(T) void k_to_live(const double* x, double* live, int n, int64_t ld) {
    const int j = blockIdx.x * T + threadIdx.x, i = blockIdx.y;
    if (j >= n || i >= j) return;
    const int64_t k = ((int64_t)(2 * n - i - 1) * i) / 2 + (j - i - 1);  // row-major index of (i, j), i < j
    const double v = (i >= 1) ? x[(int64_t)(i - 1) * ld + (j - 1)] : x[(int64_t)(j - 1) * ld + (n - 1)];
    live[k] = v;
}

// the weights above `thr` (live index order, FastNN.java:455), appended in any order: {index, weight}; *count receives their number
__global__ __launch_bounds__(T) void k_pick_positive(const double* live, int64_t N, double thr, int64_t* idx, double* w, unsigned long long* count, unsigned long long cap) {
    const int64_t k = (int64_t)blockIdx.x * T + threadIdx.x;
    const bool take = k < N && live[k] > thr;
    const unsigned long long ball = __ballot(take);
    if (ball == 0) return;
    const int lane = threadIdx.x & 63, first = __ffsll((long long)ball) - 1;
    unsigned long long base = 0;
    if (lane == first) base = atomicAdd(count, (unsigned long long)__popcll(ball));
    base = __shfl(base, first, 64);
    if (take) {
        const unsigned long long at = base + __popcll(ball & ((1ULL << lane) - 1ULL));
        if (at < cap) { idx[at] = k; w[at] = live[k]; }
    }
}
// The solver's own Kuhn-Tucker check of the returned weights (g = A^T (A x - d) from the implicit operators): per workgroup
// {max -x, max |g| over x > 0, max -g over x <= 0, max |c|} over the strict upper triangle
__global__ __launch_bounds__(T) void k_kkt(const double* x, const double* g, const double* c, int n, int64_t ld, double* partial) {
    __shared__ double sh[T / 64][4];
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    for (int i = blockIdx.y; i < n; i += gridDim.y)
        for (int j = blockIdx.x * T + threadIdx.x; j < n; j += gridDim.x * T) {
            if (i >= j) continue;
            const int64_t k = (int64_t)i * ld + j;
            const double xv = x[k], gv = g[k], cv = fabs(c[k]);
            if (-xv > v0 || xv != xv) v0 = xv != xv ? INFINITY : -xv;
            if (xv > 0.0) { if (fabs(gv) > v1 || gv != gv) v1 = gv != gv ? INFINITY : fabs(gv); }
            else if (-gv > v2 || gv != gv) v2 = gv != gv ? INFINITY : -gv;
            if (cv > v3) v3 = cv;
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v0 = fmax(v0, __shfl_down(v0, off, 64)); v1 = fmax(v1, __shfl_down(v1, off, 64));
        v2 = fmax(v2, __shfl_down(v2, off, 64)); v3 = fmax(v3, __shfl_down(v3, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { double* q = sh[threadIdx.x >> 6]; q[0] = v0; q[1] = v1; q[2] = v2; q[3] = v3; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double m = sh[0][threadIdx.x];
        for (int q = 1; q < T / 64; q++) m = fmax(m, sh[q][threadIdx.x]);
        partial[4 * (blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = m;
    }
}
// test hook (FNN_SW_FAULT_PERTURB=1): the first positive weight of the grid is doubled, so that the call's own check has something to find
__global__ void k_fault_perturb(double* x, int n, int64_t ld) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            if (x[(int64_t)i * ld + j] > 0.0) { x[(int64_t)i * ld + j] *= 2.0; return; }
}
// a = a - c over the strict upper triangle
__global__ __launch_bounds__(T) void k_sub(double* a, const double* c, int n, int64_t ld) {
    const int j = blockIdx.x * T + threadIdx.x, i = blockIdx.y;
    if (j >= n || i >= j) return;
    const int64_t k = (int64_t)i * ld + j;
    a[k] -= c[k];
}

// ---------------------------------------------------------------- "from below": block active-set method on the normal equations
// The reference's method starts from the unconstrained optimum (every split free) and contracts; on distances that are
// far from circular (random matrices: only ~2.4 n of the n(n-1)/2 splits end up with a positive weight) almost all of its
// work is conjugate-gradient iterations on huge, ill-conditioned free sets.  Lawson & Hanson's active-set method - what the
// reference's LIVE path runs (edu.rit.numeric.NonNegativeLeastSquares, FastNN.java:401-454) - grows the free set F from
// nothing and solves each sub-problem exactly.  Round 2 let ONE split enter per step (4.2 n steps, level-2 work and six
// host round trips each: 2-3.5 h at 32768 taxa).  Here whole BLOCKS enter and leave:
//   * candidates are the local maxima of the multiplier w = A^T (d - A x) on the (i, j) grid (w is smooth there: the
//     largest values sit in clusters of nearly identical splits, of which at most one survives), the largest ~10 % |F| of them;
//   * the free set's normal equations H_FF = L L^T are held as W = L^-1 (lower triangular): a block that enters appends
//     rows to W and never touches existing entries (two triangular GEMMs, one small Cholesky) - numerically benign, unlike
//     the explicitly updated inverse of round 2, whose errors compound per update;
//   * a split that leaves is not eliminated but CONSTRAINED to zero: with Y = W[:, R] the columns of the splits R that
//     left, the sub-problem's solution is x = W^T (z - Y (Y^T Y)^-1 Y^T z), z = W c - a projection, exact and stable;
//     when R exceeds ~15 % of the factor the factor is rebuilt from H's closed form (Cholesky + triangular inverse);
//   * all splits with a negative weight leave at once; the step is kept only if the objective -c_F.x_F/2 fell, otherwise
//     the block is taken back (the appended rows are simply dropped), shrunk, and at a single split the Lawson-Hanson
//     ratio step - whose descent is guaranteed - takes over.
// H has a closed form: the number of position pairs that two circular splits S, T both separate is
// |S n T| |S^c n T^c| + |S n T^c| |S^c n T|.
__device__ __forceinline__ double h_entry(int n, int i, int j, int k, int l) {  // splits (i,j), (k,l): positions {i+1..j}, {k+1..l}
    const int lo = i > k ? i : k, hi = j < l ? j : l;
    const double st = hi > lo ? (double)(hi - lo) : 0.0, s = (double)(j - i), t = (double)(l - k);
    return st * ((double)n - s - t + st) + (s - st) * (t - st);
}
// out[r + c ldo] = H[Fa[r], Fb[c]] (column-major); lower_only: entries above the diagonal are written as zeros
__global__ __launch_bounds__(T) void k_hblock(const int2* Fa, int64_t fa, const int2* Fb, int64_t fb, int n, double* out, int64_t ldo,
                                              int lower_only) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r >= fa) return;
    const int2 a = Fa[r];
    for (int64_t c = blockIdx.y; c < fb; c += gridDim.y) {
        const int2 b = Fb[c];
        out[c * ldo + r] = (lower_only && r < c) ? 0.0 : h_entry(n, a.x, a.y, b.x, b.y);
    }
}
__global__ __launch_bounds__(T) void k_gather(const int2* F, int64_t f, const double* grid, int64_t ld, double* out) {
    const int64_t p = (int64_t)blockIdx.x * T + threadIdx.x;
    if (p < f) out[p] = grid[(int64_t)F[p].x * ld + F[p].y];
}
__global__ __launch_bounds__(T) void k_scatter(const int2* F, int64_t f, const double* v, double* grid, int64_t ld) {
    const int64_t p = (int64_t)blockIdx.x * T + threadIdx.x;
    if (p < f) grid[(int64_t)F[p].x * ld + F[p].y] = v[p];
}
__global__ __launch_bounds__(T) void k_mask(const int2* F, int64_t f, uint8_t* mask, int64_t ld, uint8_t v) {
    const int64_t p = (int64_t)blockIdx.x * T + threadIdx.x;
    if (p < f) mask[(int64_t)F[p].x * ld + F[p].y] = v;
}
// A lower-triangular inverse factor as COLUMN PANELS of width pw: panel q holds the rows [q pw, cap) of its pw columns,
// column-major with leading dimension cap - q pw - the zero half above the diagonal blocks is not stored (half the memory
// of a square - 9/16 with the eight panels used - which is what bounds the factor's capacity at 32768 taxa).  Every product with
// the factor runs panel by panel.  pw >= cap: one panel = plain square storage (the Gram factor of the departed columns).
struct TriStore {
    double* base;
    int64_t cap, pw;
    __host__ __device__ int64_t off(int64_t q) const { return pw * (q * cap - pw * (q * (q - 1) / 2)); }
    __host__ __device__ int64_t ld(int64_t q) const { return cap - q * pw; }
    __host__ __device__ double* panel(int64_t q) const { return base + off(q); }
    __host__ __device__ double* at(int64_t row, int64_t col) const {  // row >= the first row of the column's panel
        const int64_t q = col / pw, q0 = q * pw;
        return base + off(q) + (col - q0) * ld(q) + (row - q0);
    }
};  // (its size in doubles: tri_elems of fnn_splits_plan.h)
// Y[:, q] = W[0:f, list[q]] for a panel-stored factor (rows above the column's panel are zeros)
__global__ __launch_bounds__(T) void k_gather_cols_tri(TriStore W, int64_t f, const int32_t* list, int64_t cnt, double* Y, int64_t ldy) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r >= f) return;
    for (int64_t q = blockIdx.y; q < cnt; q += gridDim.y) {
        const int64_t c = list[q];
        Y[q * ldy + r] = r >= (c / W.pw) * W.pw ? *W.at(r, c) : 0.0;
    }
}
// Y[f0 + i, q] = W[f0 + i, list[q]], i < k (list[q] < f0: the rows lie inside the columns' panels)
__global__ __launch_bounds__(T) void k_gather_rows_tri(TriStore W, int64_t f0, int64_t k, const int32_t* list, int64_t cnt, double* Y, int64_t ldy) {
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
    if (i >= k) return;
    for (int64_t q = blockIdx.y; q < cnt; q += gridDim.y) Y[q * ldy + f0 + i] = *W.at(f0 + i, list[q]);
}
// Y[:, q] = W[0:f, list[q]] (columns of the splits that left)
__global__ __launch_bounds__(T) void k_gather_cols(const double* W, int64_t ldw, int64_t f, const int32_t* list, int64_t cnt, double* Y, int64_t ldy) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r >= f) return;
    for (int64_t q = blockIdx.y; q < cnt; q += gridDim.y) Y[q * ldy + r] = W[(int64_t)list[q] * ldw + r];
}
// out (m x m, ldo) = a[idx, idx] (a: lda), the sub-block of the kept rows / columns
__global__ __launch_bounds__(T) void k_gather_sym(const double* a, int64_t lda, const int32_t* idx, int64_t m, double* out, int64_t ldo) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r >= m) return;
    const int64_t ri = idx[r];
    for (int64_t c = blockIdx.y; c < m; c += gridDim.y) out[c * ldo + r] = a[(int64_t)idx[c] * lda + ri];
}
__global__ __launch_bounds__(T) void k_gather_vec(const double* a, const int32_t* idx, int64_t m, double* out) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r < m) out[r] = a[idx[r]];
}
__global__ __launch_bounds__(T) void k_gather_int2(const int2* a, const int32_t* idx, int64_t m, int2* out) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r < m) out[r] = a[idx[r]];
}
// out (nn x m, ldo) = a^T (a: m x nn, lda)
__global__ __launch_bounds__(T) void k_transpose_small(const double* a, int64_t lda, int64_t m, int64_t nn, double* out, int64_t ldo) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;  // row of a
    if (r >= m) return;
    for (int64_t c = blockIdx.y; c < nn; c += gridDim.y) out[r * ldo + c] = a[c * lda + r];
}
// copy the lower triangle of a (m x m, lda) into b (ldb), zeros above the diagonal
__global__ __launch_bounds__(T) void k_copy_lower(const double* a, int64_t lda, double* b, int64_t ldb, int64_t m) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r >= m) return;
    for (int64_t c = blockIdx.y; c < m; c += gridDim.y) b[c * ldb + r] = r >= c ? a[c * lda + r] : 0.0;
}
// rows x cols block (column-major: the rows of a column are adjacent) filled / copied by kernels: the runtime's 2-D fill
// (hipMemset2DAsync -> fillBufferAligned2D) ran at 6 GB/s on the pitched blocks of the factor - 209 ms for the 1.2 GB of zeros
// above a block's new columns, 6.8 s of a 32768-taxon solve (profiles/r03/r03_splits_kernel_stats_n32768.csv) - and the 2-D
// device-to-device copies go through the copy engines.
__global__ __launch_bounds__(T) void k_fill2d(double* dst, int64_t ldd, int64_t rows, int64_t cols, double v) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r >= rows) return;
    for (int64_t c = blockIdx.y; c < cols; c += gridDim.y) dst[c * ldd + r] = v;
}
__global__ __launch_bounds__(T) void k_copy2d(const double* src, int64_t lds_, double* dst, int64_t ldd, int64_t rows, int64_t cols) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r >= rows) return;
    for (int64_t c = blockIdx.y; c < cols; c += gridDim.y) dst[c * ldd + r] = src[c * lds_ + r];
}
constexpr int TRI_NB = 64;
// inverse of the Cholesky factor of a symmetric positive definite m x m block (m <= 64; lower triangle of S read):
// Li (lower triangular, zeros above) with Li^T Li = S^-1.  ONE wave; lane t owns ROW t of the matrix in registers (every index
// below is a compile-time constant: the loops are unrolled, 256 VGPR, no scratch); the entry of another row that a step needs
// is the same for all lanes and comes straight out of the owning lane's register (two v_readlane_b32 into a scalar pair
// that feeds the FMA): no LDS round trip on the 4032 multiply-adds.  Left-looking Cholesky, then lane t computes COLUMN t of
// the inverse by forward substitution.  Measured (profiles/r03/r03_splits_kernel_stats_n4096.csv): 64 us per block - a first
// version that walked an LDS copy with dependent reads took 170 us (45 % of a 4096-taxon solve).  What bounds it now is the
// fetch of its own ~100 KB of straight-line code, executed once per launch (the same 64 us with broadcast LDS reads in place of
// the lane reads); a rolled loop would index the register rows at run time, at about the same cost per term.
// Rows beyond m are padded with the identity.  A pivot that is not positive reports its (1-based, offset by `off`)
// position through atomicMin on *info.  (Not on the bit-exact path: FMAs are welcome here.)
__device__ __forceinline__ double lane_value(double v, int src) {  // the value lane `src` holds (src a compile-time constant)
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__global__ __launch_bounds__(TRI_NB) void k_invchol_small(const double* S, int64_t lds, double* Li, int64_t ldl, int m, long long off, long long* info) {
    __shared__ double Ls[TRI_NB][TRI_NB + 1];
    __shared__ double rd[TRI_NB];
    const int t = threadIdx.x;
    double a[TRI_NB];
#pragma unroll
    for (int c = 0; c < TRI_NB; c++) a[c] = (t < m && c <= t) ? S[(int64_t)c * lds + t] : (c == t ? 1.0 : 0.0);
#pragma unroll
    for (int j = 0; j < TRI_NB; j++) {
        double sj = a[j];
#pragma unroll
        for (int l = 0; l < j; l++) sj = __builtin_fma(-a[l], lane_value(a[l], j), sj);  // (row t) . (row j) over the finished columns
        double piv = lane_value(sj, j);
        if (!(piv > 0.0)) {
            if (t == j && j < m) atomicMin(info, off + j + 1);
            piv = 1.0;
        }
        const double dj = __builtin_sqrt(piv);
        a[j] = t == j ? dj : (t > j ? sj / dj : 0.0);
        if (t == j) rd[j] = 1.0 / dj;
    }
    __syncthreads();
    // column t of L^-1: x_i = (delta_it - sum_{l < i} L_il x_l) / L_ii (x_l = 0 for l < t falls out of the recurrence)
    double x[TRI_NB];
#pragma unroll
    for (int i = 0; i < TRI_NB; i++) {
        double acc = i == t ? 1.0 : 0.0;
#pragma unroll
        for (int l = 0; l < i; l++) acc = __builtin_fma(-lane_value(a[l], i), x[l], acc);
        x[i] = acc * rd[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TRI_NB; i++) Ls[i][t] = x[i];  // X[i][t]
    __syncthreads();
    for (int c = 0; c < m; c++)
        if (t < m) Li[(int64_t)c * ldl + t] = Ls[t][c];
}
// local maxima of the multiplier on the (i, j) grid: entry (i, j), i < j, not masked, w > tol, and no unmasked neighbour
// within `rad` (Chebyshev) is larger in the order (w, index).  Winners are appended to the candidate list.
__global__ __launch_bounds__(T) void k_candidates(const double* w, const uint8_t* mask, int n, int64_t ld, double tol, int rad,
                                                  double* key, int64_t* idx, unsigned long long* count, unsigned long long capacity) {
    const int j = blockIdx.x * T + threadIdx.x, i = blockIdx.y;
    bool win = false;
    int64_t k = 0;
    double v = 0.0;
    if (j < n && i < j) {
        k = (int64_t)i * ld + j;
        v = w[k];
        if (!mask[k] && v > tol) {
            win = true;
            for (int di = -rad; di <= rad && win; di++) {
                const int ii = i + di;
                if (ii < 0 || ii >= n) continue;
                for (int dj = -rad; dj <= rad; dj++) {
                    const int jj = j + dj;
                    if ((di == 0 && dj == 0) || jj <= ii || jj >= n) continue;
                    const int64_t kk = (int64_t)ii * ld + jj;
                    const double u = w[kk];
                    if (!mask[kk] && (u > v || (u == v && kk < k))) { win = false; break; }
                }
            }
        }
    }
    const unsigned long long ball = __ballot(win);
    if (ball == 0) return;
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (lane == __ffsll((long long)ball) - 1) base = atomicAdd(count, (unsigned long long)__popcll(ball));
    base = __shfl(base, __ffsll((long long)ball) - 1, 64);
    if (win) {
        const unsigned long long at = base + __popcll(ball & ((1ULL << lane) - 1ULL));
        if (at < capacity) { key[at] = v; idx[at] = k; }
    }
}
// C (m x nn, ldc) = beta C + alpha * sum over the `parts` partial products at P + q * stride (each m x nn, ld m)
__global__ __launch_bounds__(T) void k_sum_parts(const double* P, int64_t stride, int parts, int64_t m, int64_t nn, double alpha, double beta, double* C,
                                                 int64_t ldc) {
    const int64_t r = (int64_t)blockIdx.x * T + threadIdx.x;
    if (r >= m) return;
    for (int64_t c = blockIdx.y; c < nn; c += gridDim.y) {
        double acc = 0.0;
        for (int q = 0; q < parts; q++) acc += P[(int64_t)q * stride + c * m + r];
        C[c * ldc + r] = (beta == 0.0 ? 0.0 : beta * C[c * ldc + r]) + alpha * acc;
    }
}
// A block of at most SMALLK columns: out (f x k) = Wl (lower triangular) * Bm, Wl read once.  One thread per row, a
// workgroup per 256 rows and column chunk; partial sums per chunk, added up in chunk order by k_sum_parts.
constexpr int SMALLK = 8;
constexpr int SK_CHUNK = 2048;
__global__ __launch_bounds__(T) void k_tri_times_small(TriStore Wl, int64_t f, const double* Bm, int64_t ldb, int k, double* part) {
    const int64_t row = (int64_t)blockIdx.x * T + threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.y * SK_CHUNK;
    if ((int64_t)blockIdx.x * T + T - 1 < c0) return;  // the whole row block lies above the diagonal of this chunk: zeros (the buffer is cleared)
    double acc[SMALLK];
#pragma unroll
    for (int a = 0; a < SMALLK; a++) acc[a] = 0.0;
    if (row < f) {
        int64_t c1 = c0 + SK_CHUNK < f ? c0 + SK_CHUNK : f;
        if (row + 1 < c1) c1 = row + 1;
        for (int64_t c = c0; c < c1; c++) {
            const double w = *Wl.at(row, c);
#pragma unroll
            for (int a = 0; a < SMALLK; a++)
                if (a < k) acc[a] += w * Bm[(int64_t)a * ldb + c];
        }
#pragma unroll
        for (int a = 0; a < SMALLK; a++)
            if (a < k) part[((int64_t)blockIdx.y * k + a) * f + row] = acc[a];
    }
}
// out (k x f, ldo) = Tm^T (f x k) * Wl (lower triangular): one workgroup per column of Wl, Wl read once
__global__ __launch_bounds__(T) void k_t_times_tri_small(const double* Tm, int64_t ldt, int k, TriStore Wl, int64_t f, double* out, int64_t ldo) {
    __shared__ double sh[T / 64][SMALLK];
    const int64_t j = blockIdx.x;
    double acc[SMALLK];
#pragma unroll
    for (int a = 0; a < SMALLK; a++) acc[a] = 0.0;
    const double* colj = Wl.at(j, j) - 0;  // column j from its diagonal entry down (contiguous inside its panel)
    for (int64_t l = j + threadIdx.x; l < f; l += T) {
        const double w = colj[l - j];
#pragma unroll
        for (int a = 0; a < SMALLK; a++)
            if (a < k) acc[a] += w * Tm[(int64_t)a * ldt + l];
    }
#pragma unroll
    for (int a = 0; a < SMALLK; a++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[a] += __shfl_down(acc[a], off, 64);
    }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < SMALLK; a++) sh[threadIdx.x >> 6][a] = acc[a];
    __syncthreads();
    if (threadIdx.x < k) out[j * ldo + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}
__global__ __launch_bounds__(T) void k_idx_to_split(const int64_t* idx, int64_t cnt, int64_t ld, int2* out) {
    const int64_t p = (int64_t)blockIdx.x * T + threadIdx.x;
    if (p < cnt) out[p] = make_int2((int)(idx[p] / ld), (int)(idx[p] % ld));
}

// ---------------------------------------------------------------- device buffers kept between calls
// hipMalloc of the solver's ~220 GB costs 0.5-4.8 s from box to box (page tables: `fnn_sw_stats.t_alloc_s`).  Buffers of >= 64 MiB
// go back to a per-process pool instead of the driver and are handed out again to a request of exactly that size on that
// device (a second solve of the same n: every one of them); a failed hipMalloc - or a caller who wants the memory,
// fnn_split_weights_release_cache - empties the pool.  The pool's bytes count as free when the factor is sized.
struct BufferPool {
    struct Item { void* p; size_t bytes; int dev; };
    std::vector<Item> items;
    std::mutex mu;
    static constexpr size_t kMin = (size_t)64 << 20;
    void* take(size_t bytes, int dev) {
        std::lock_guard<std::mutex> g(mu);
        for (size_t i = 0; i < items.size(); i++)
            if (items[i].bytes == bytes && items[i].dev == dev) { void* p = items[i].p; items.erase(items.begin() + (long)i); return p; }
        return nullptr;
    }
    void give(void* p, size_t bytes, int dev) {
        if (bytes < kMin) { (void)hipFree(p); return; }
        std::lock_guard<std::mutex> g(mu);
        items.push_back(Item{p, bytes, dev});
    }
    size_t pooled(int dev) {
        std::lock_guard<std::mutex> g(mu);
        size_t t = 0;
        for (const Item& it : items) if (it.dev == dev) t += it.bytes;
        return t;
    }
    void flush() {
        std::lock_guard<std::mutex> g(mu);
        for (const Item& it : items) (void)hipFree(it.p);
        items.clear();
    }
};
inline BufferPool& pool() { static BufferPool* p = new BufferPool; return *p; }  // (never destroyed: no hipFree after the runtime has gone)

// ---------------------------------------------------------------- host driver
struct Solver {
    int n = 0;
    int64_t ld = 0;
    hipStream_t s = nullptr;
    std::vector<void*> allocs;
    std::vector<size_t> alloc_bytes;  // (parallel to allocs)
    int dev = 0;
    double *d = nullptr, *x = nullptr, *r = nullptr, *w = nullptr, *p = nullptr, *y = nullptr, *old_x = nullptr, *atwd = nullptr;
    double *P = nullptr, *Pt = nullptr, *rs = nullptr, *partial = nullptr, *live = nullptr, *Dm = nullptr, *sc = nullptr;
    int32_t* ord = nullptr;
    uint8_t* act = nullptr;
    Best* bpartial = nullptr;
    dim3 grid2, gred;
    int64_t st_outer = 0, st_cg = 0, st_it = 0;
    bool ok = true;

    template <class Tp>
    Tp* alloc(size_t count) {
        const size_t bytes = sizeof(Tp) * (count ? count : 1);
        void* p_ = pool().take(bytes, dev);
        if (!p_ && !SWOK(hipMalloc(&p_, bytes))) {
            (void)hipGetLastError();
            pool().flush();  // (what the pool holds may be what is missing)
            if (!SWOK(hipMalloc(&p_, bytes))) { ok = false; return nullptr; }
        }
        allocs.push_back(p_);
        alloc_bytes.push_back(bytes);
        return (Tp*)p_;
    }
    void release(void* p_) {  // one allocation back to the device (after the work queued on it)
        (void)hipStreamSynchronize(s);
        for (size_t i = 0; i < allocs.size(); i++)
            if (allocs[i] == p_) { pool().give(p_, alloc_bytes[i], dev); allocs.erase(allocs.begin() + (long)i); alloc_bytes.erase(alloc_bytes.begin() + (long)i); return; }
    }
    size_t block_mark = SIZE_MAX;  // allocs[block_mark ..) belong to the block active-set method
    void release_block_buffers() {
        (void)hipStreamSynchronize(s);
        if (block_mark == SIZE_MAX) return;
        while (allocs.size() > block_mark) { pool().give(allocs.back(), alloc_bytes.back(), dev); allocs.pop_back(); alloc_bytes.pop_back(); }
        ok = true;
    }
    ~Solver() {
        if (s) (void)hipStreamSynchronize(s);
        for (size_t i = 0; i < allocs.size(); i++) pool().give(allocs[i], alloc_bytes[i], dev);
        if (s) (void)hipStreamDestroy(s);
    }
    // 2-D inclusive prefix of src (upper triangle, zeros elsewhere) -> Pt (transposed)
    void prefix(const double* src, const double* skip) {
        hipLaunchKernelGGL(k_rowscan, dim3(n), dim3(T), 0, s, src, P, n, ld, skip);
        hipLaunchKernelGGL(k_transpose, dim3((n + 31) / 32, (n + 31) / 32), dim3(T), 0, s, P, Pt, n, ld, skip);
        hipLaunchKernelGGL(k_rowscan, dim3(n), dim3(T), 0, s, Pt, Pt, n, ld, skip);
    }
    void Ab(const double* b_, double* out, const double* skip = nullptr) {  // out = A b
        prefix(b_, skip);
        hipLaunchKernelGGL(k_ab, grid2, dim3(T), 0, s, Pt, out, n, ld, skip);
    }
    void Atx(const double* y_, double* out, const uint8_t* mask = nullptr, const double* skip = nullptr) {  // out = A^T y
        prefix(y_, skip);
        hipLaunchKernelGGL(k_scan1, dim3(1), dim3(1024), 0, s, Pt, rs, n, ld, skip);
        hipLaunchKernelGGL(k_atx, grid2, dim3(T), 0, s, Pt, rs, out, n, ld, mask, skip);
    }
    template <int OP>
    void vec(double* a, double* b, const double* c, const double* e, double s0 = 0.0, double s1 = 0.0, const double* scp = nullptr) {
        VecArgs g{a, b, c, e, act, s0, s1, n, ld, scp};
        hipLaunchKernelGGL(k_vec<OP>, grid2, dim3(T), 0, s, g);
    }
    void dot_partials(const double* a, const double* b, const double* skip) {
        hipLaunchKernelGGL(k_reduce<RD_DOT>, gred, dim3(T), 0, s, a, b, act, 0.0, n, ld, partial, bpartial, skip);
    }
    // the per-workgroup partials of the reduction just launched, on the host (the three folds below are their callers' own)
    template <class Tp>
    std::vector<Tp> fetch_partials(const Tp* dev) {
        std::vector<Tp> h((size_t)gred.x * gred.y);
        (void)hipMemcpyAsync(h.data(), dev, sizeof(Tp) * h.size(), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        return h;
    }
    template <int RD>
    double reduce_sum(const double* a, const double* b, double s0 = 0.0) {
        hipLaunchKernelGGL(k_reduce<RD>, gred, dim3(T), 0, s, a, b, act, s0, n, ld, partial, bpartial, (const double*)nullptr);
        double acc = 0.0;
        for (double v : fetch_partials(partial)) acc += v;
        return acc;
    }
    template <int RD>
    Best reduce_best(const double* a, const double* b) {
        hipLaunchKernelGGL(k_reduce<RD>, gred, dim3(T), 0, s, a, b, act, 0.0, n, ld, partial, bpartial, (const double*)nullptr);
        Best best{INFINITY, INT64_MAX};
        for (const Best& o : fetch_partials(bpartial))
            if (o.v < best.v || (o.v == best.v && o.k < best.k)) best = o;
        return best;
    }
    double min_negative(const double* a) {
        hipLaunchKernelGGL(k_minneg, gred, dim3(T), 0, s, a, n, ld, partial);
        double mn = 0.0;
        for (double v : fetch_partials(partial)) if (v < mn) mn = v;
        return mn;
    }

    // circularConjugateGrads (:769-831), W = 1.  The loop's scalars stay on the device; the host enqueues
    // CG_CHECK iterations at a time and reads the loop condition once per bunch (the kernels of an
    // iteration that comes after the end of the loop return at once, so the iteration count is exactly
    // the reference's).
    static constexpr int CG_CHECK = 16;
    double tol2 = -1.0;  // (CG_EPSILON * ||AtWd||)^2, constant over the solve
    void cg() {
        const int np = (int)(gred.x * gred.y);
        if (tol2 < 0.0) { const double e_0 = CG_EPSILON * std::sqrt(reduce_sum<RD_DOT>(atwd, atwd)); tol2 = e_0 * e_0; }
        double hsc[SC_WORDS] = {0};
        hsc[SC_TOL2] = tol2;
        hsc[SC_KMAX] = (double)((int64_t)n * (n - 1) / 2);
        (void)hipMemcpyAsync(sc, hsc, sizeof(hsc), hipMemcpyHostToDevice, s);
        (void)hipStreamSynchronize(s);  // (hsc is a stack buffer)
        Ab(x, y);
        Atx(y, r);
        vec<OP_R_INIT>(r, nullptr, atwd, nullptr);
        dot_partials(r, r, nullptr);
        hipLaunchKernelGGL(k_cg_scalar, dim3(1), dim3(T), 0, s, partial, np, sc, 0);
        for (;;) {
            for (int it = 0; it < CG_CHECK; it++) {
                vec<OP_P_UPDATE>(p, nullptr, r, nullptr, 0.0, 0.0, sc);
                Ab(p, y, sc);
                Atx(y, w, act, sc);
                dot_partials(p, w, sc);
                hipLaunchKernelGGL(k_cg_scalar, dim3(1), dim3(T), 0, s, partial, np, sc, 1);
                vec<OP_XR_UPDATE>(x, r, p, w, 0.0, 0.0, sc);
                dot_partials(r, r, sc);
                hipLaunchKernelGGL(k_cg_scalar, dim3(1), dim3(T), 0, s, partial, np, sc, 2);
            }
            (void)hipMemcpyAsync(hsc, sc, sizeof(hsc), hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            if (hsc[SC_DONE] != 0.0) break;
        }
        st_cg++;
        st_it += (int64_t)hsc[SC_K];
    }
    // worstIndices(x, 0.6) + contraction (:411-430).  Returns false if nothing is negative.
    bool contract_worst() {
        const int64_t num_neg = (int64_t)reduce_sum<RD_COUNT_NEG>(x, nullptr);
        if (num_neg == 0) return false;
        const int64_t nkept = (int64_t)std::ceil(0.6 * (double)num_neg);
        // cutoff = nkept-th smallest negative value.  count(x < t) is monotone in t; bisect over the
        // bit patterns of the negative doubles (larger pattern = more negative), at most 64 steps:
        // invariant count(x < val(lo)) < nkept <= count(x < val(hi)), lo more negative than hi
        auto val = [](uint64_t bits) { double v; std::memcpy(&v, &bits, 8); return v; };
        const double mn = min_negative(x);
        uint64_t lo, hi = 0x8000000000000000ULL;  // hi = -0.0: count(x < -0.0) = num_neg >= nkept
        std::memcpy(&lo, &mn, 8);                  // count(x < min) = 0 < nkept
        while (lo - hi > 1) {
            const uint64_t mid = hi + (lo - hi) / 2;
            const int64_t c = (int64_t)reduce_sum<RD_COUNT_LT>(x, nullptr, val(mid));
            if (c >= nkept) hi = mid; else lo = mid;
        }
        // no double lies strictly between val(lo) and val(hi): the nkept-th smallest value is val(lo).
        // Values below it all go; of the values equal to it the reference takes the first
        // nkept - count(<) by index - here they are taken together (the same unless equal negative
        // weights straddle the 60 % mark; the optimum reached does not depend on it)
        vec<OP_CONTRACT>(x, nullptr, nullptr, nullptr, val(lo), 1.0);
        return true;
    }

    // ------------------------------------------------------------ what the block active-set method (BlockMethod, below) leaves here
    // A call may make several attempts at growing capacities, each a fresh BlockMethod: the counters, the timers, gemm_flops and
    // f_peak ACCUMULATE over the attempts of one call; giveup, capacity and t_alloc_s are the last attempt's.
    int64_t st_lh_steps = 0, st_lh_refactor = 0, st_solves = 0, st_adds = 0, st_dels = 0, st_rejects = 0, st_ratio_steps = 0, st_screened = 0, st_dead_wanting = 0, st_revived = 0, st_dels_new = 0;
    double t_ops = 0, t_sel = 0, t_append = 0, t_solve = 0, t_dead = 0, t_refactor = 0;  // host wall clock per phase (FNN_SW_LOG)
    double gemm_flops = 0.0;
    int64_t cap_want = 0;        // > 0: the factor's capacity for this attempt (a retry after FNN_SW_GIVEUP_CAPACITY), else the default for n
    int giveup = 0;              // FNN_SW_GIVEUP_* of the block method
    const char* giveup_text = "";
    double final_tol_rel = 0.0, t_alloc_s = 0.0;
    int64_t n_set_aside = 0, f_peak = 0, capacity = 0;
    bool have_atwd = false;
    double wall() { (void)hipStreamSynchronize(s); return fnn::now_s(); }
    std::map<std::string, double> tsub;  // finer split of the phases (FNN_SW_LOG)
    double t_lap = 0.0;
    bool lap_on = false;
    void lap(const char* name) {
        if (!lap_on) return;
        const double t = wall();
        if (name) tsub[name] += t - t_lap;
        t_lap = t;
    }

    // ---------------------------------------------------------------- the block active-set method (see the comment above h_entry)
    // One attempt at one capacity.  The state is grouped by what owns it - the factor, the departed columns, the candidates,
    // scratch, the policy of the step loop -; run() is the step loop, a sequence of named steps.  The implicit operators, the
    // reductions, the allocator, the stream and the counters that outlive an attempt are the Solver's.
    struct BlockMethod {
        Solver& sv;
        const Knobs& kn;
        const int n;
        const int64_t ld, N;
        const hipStream_t s;
        const bool log;
        rocblas_handle bh = nullptr;
        bool blas_ok = true;
        bool good = true, done = false;  // good: no give-up so far; done: no candidate is left

        // The factor: the free set's normal equations H_FF = L L^T held as Ws = L^-1 (lower triangular, column panels)
        struct Factor {
            std::vector<int2> F;     // the factor's splits in factor order
            std::vector<double> xw;  // weight per factor position (0 for the splits that left)
            std::vector<double> cF;  // c = A^T d at the factor positions
            int64_t f = 0, cap = 0, kmax = 0, pw = 0;  // splits inside, capacity, the largest block, panel width
            TriStore Ws{nullptr, 0, 0};
            int2* dF = nullptr;      // F on the device
            double *z = nullptr, *xs = nullptr, *cK = nullptr, *gF = nullptr;  // z = W c; the sub-problem's solution; c and A^T A x at splits
        } fac;
        // The departed columns: the splits that left are constrained to zero, not eliminated
        struct Departed {
            std::vector<uint8_t> dead;      // per factor position
            std::vector<int32_t> deadlist;  // factor positions of the splits that left, in the order of Y's columns
            int64_t r = 0, rcap = 0;
            double *Y = nullptr, *CR = nullptr, *LC = nullptr, *CRb = nullptr, *CRw = nullptr;  // Y = W[:, R], its Gram matrix, the Gram factor; copies
            TriStore LCs{nullptr, 0, 0};    // (LC as one panel = square)
            double* lam = nullptr;
            int32_t* dlist = nullptr;       // deadlist on the device
        } dep;
        // The candidates: local maxima of the multiplier, unsorted and sorted
        struct Candidates {
            double *ckey = nullptr, *ckey2 = nullptr;
            int64_t *cidx = nullptr, *cidx2 = nullptr;
            unsigned long long* ccount = nullptr;
            void* sort_tmp = nullptr;
            size_t sort_bytes = 0;
            int64_t ccap = 0;
        } cand;
        // Scratch: nothing here outlives the call that fills it
        struct Scratch {
            double *B = nullptr, *Tb = nullptr, *X = nullptr, *S = nullptr, *S0 = nullptr, *Li = nullptr, *tmp2 = nullptr;
            int2* dscr = nullptr;
            int32_t* dlist2 = nullptr;
            double *wk = nullptr, *sk1 = nullptr, *sk2 = nullptr, *v = nullptr;
            int64_t* dinfo = nullptr;
        } scr;
        // The policy of the step loop: everything a rule of run() reads or changes
        struct Policy {
            double tol = 0.0, tol_cap = 0.0, cmax = 0.0;  // multipliers above tol are candidates (raised to the measured noise floor, up to tol_cap)
            double phi = 0.0;               // objective - c_F . x_F / 2 of the current point (a sub-problem's exact minimiser)
            int64_t k_limit = 0, kmin = 0;
            double rfrac_buf = 0.0;
            bool ratio_mode = false;
            bool fresh = false;             // the point comes straight from a rebuilt factor
            int stall = 0;                  // steps in a row whose descent is not measurable (below 1e-13 |objective|)
            std::vector<int2> banned;       // splits set aside: masked, but not in the factor
            bool banned_rechecked = false;
            bool revive_blocked = false;    // a step that only brought departed splits back did not descend: not again before a step moves
            bool force_rebuild = false;     // a step ran out of room for its departed columns (taken back): rebuild before the next one
            bool over_rcap = false;         // settle_all failed for lack of room for the departed columns (not a numerical failure)
            int64_t f_step0 = 0;            // (statistics: factor size before this step's block entered)
        } pol;
        std::vector<double> sbuf;           // the minimiser of the last sub-problem solved

        BlockMethod(Solver& solver, const Knobs& knobs)
            : sv(solver), kn(knobs), n(solver.n), ld(solver.ld), N((int64_t)solver.n * (solver.n - 1) / 2), s(solver.s), log(knobs.log) {}
        ~BlockMethod() { if (bh) rocblas_destroy_handle(bh); }
        BlockMethod(const BlockMethod&) = delete;

        static dim3 g1(int64_t c) { return dim3((unsigned)((c + T - 1) / T)); }
        static dim3 g2(int64_t rows, int64_t cols) { return dim3((unsigned)((rows + T - 1) / T), (unsigned)std::max<int64_t>(1, std::min<int64_t>(cols, 16384))); }
        bool give(int why, const char* text) { sv.giveup = why; sv.giveup_text = text; good = false; return false; }

        // ------------------------------------------------------------ dense algebra on the stream
        void gemm(rocblas_operation ta, rocblas_operation tb, int64_t m, int64_t nn, int64_t k, double alpha, const double* A, int64_t lda, const double* Bm,
                  int64_t ldb, double beta, double* Cm, int64_t ldc) {
            if (m <= 0 || nn <= 0) return;
            sv.gemm_flops += 2.0 * (double)m * (double)nn * (double)k;
            if (rocblas_dgemm_64(bh, ta, tb, m, nn, k, &alpha, A, lda, Bm, ldb, &beta, Cm, ldc) != rocblas_status_success) blas_ok = false;
        }
        void gemv(rocblas_operation ta, int64_t m, int64_t nn, double alpha, const double* A, int64_t lda, const double* xv, double beta, double* yv) {
            if (m <= 0 || nn <= 0) return;
            if (rocblas_dgemv_64(bh, ta, m, nn, &alpha, A, lda, xv, 1, &beta, yv, 1) != rocblas_status_success) blas_ok = false;
        }
        // panels that skip the zero half of a lower-triangular operand
        // out (f x k, ldo) = Wl (f x f lower triangular, panel-stored) * Bm (f x k, ldb): panel by panel, each adding into the rows it reaches
        void tri_times(const TriStore& Wl, int64_t f, const double* Bm, int64_t ldb, int64_t k, double* out, int64_t ldo) {
            const int64_t chunks = (f + SK_CHUNK - 1) / SK_CHUNK;
            if (k <= SMALLK && chunks * k * f <= fac.cap * fac.kmax) {  // a few columns: one pass over Wl (partial sums per column chunk in scr.X)
                (void)hipMemsetAsync(scr.X, 0, sizeof(double) * (size_t)(chunks * k * f), s);
                hipLaunchKernelGGL(k_tri_times_small, dim3((unsigned)((f + T - 1) / T), (unsigned)chunks), dim3(T), 0, s, Wl, f, Bm, ldb, (int)k, scr.X);
                hipLaunchKernelGGL(k_sum_parts, g2(f, k), dim3(T), 0, s, scr.X, k * f, (int)chunks, f, k, 1.0, 0.0, out, ldo);
                return;
            }
            // column chunks of about f / 8 (never across a storage panel): the zero triangle above a chunk's diagonal is the only waste
            const int64_t gw = std::min(Wl.pw, std::max<int64_t>(1024, up64((f + 7) / 8)));
            for (int64_t c0 = 0; c0 < f;) {
                const int64_t q = c0 / Wl.pw, c1 = std::min({c0 + gw, (q + 1) * Wl.pw, f});
                gemm(rocblas_operation_none, rocblas_operation_none, f - c0, k, c1 - c0, 1.0, Wl.at(c0, c0), Wl.ld(q), Bm + c0, ldb, c0 == 0 ? 0.0 : 1.0, out + c0, ldo);
                c0 = c1;
            }
        }
        // out (k x f, ldo) = Tm^T (Tm: f x k, ldt) * Wl (f x f lower triangular, panel-stored)
        void t_times_tri(const double* Tm, int64_t ldt, int64_t k, const TriStore& Wl, int64_t f, double* out, int64_t ldo) {
            if (k <= SMALLK) {
                hipLaunchKernelGGL(k_t_times_tri_small, dim3((unsigned)f), dim3(T), 0, s, Tm, ldt, (int)k, Wl, f, out, ldo);
                return;
            }
            const int64_t gw = std::min(Wl.pw, std::max<int64_t>(1024, up64((f + 7) / 8)));
            for (int64_t c0 = 0; c0 < f;) {
                const int64_t q = c0 / Wl.pw, c1 = std::min({c0 + gw, (q + 1) * Wl.pw, f});
                gemm(rocblas_operation_transpose, rocblas_operation_none, k, c1 - c0, f - c0, 1.0, Tm + c0, ldt, Wl.at(c0, c0), Wl.ld(q), 0.0, out + c0 * ldo, ldo);
                c0 = c1;
            }
        }
        // C (m x nn) = beta C + alpha A^T B with a long inner dimension kk (A: kk x m, B: kk x nn): rocBLAS has no split-K form of
        // this shape (3 TF/s); here the inner dimension is cut into slices that run as one strided-batched GEMM into partial
        // products (workspace scr.X), added up in slice order
        void tn_splitk(int64_t m, int64_t nn, int64_t kk, double alpha, const double* A, int64_t lda, const double* Bm, int64_t ldb, double beta, double* Cm,
                       int64_t ldc) {
            if (m <= 0 || nn <= 0) return;
            const int64_t room = (fac.cap * fac.kmax) / std::max<int64_t>(m * nn, 1);
            int64_t parts = std::min<int64_t>({room, (int64_t)32, (kk + 1023) / 1024});
            if (parts < 2 || m * nn > (int64_t)1 << 26) {
                gemm(rocblas_operation_transpose, rocblas_operation_none, m, nn, kk, alpha, A, lda, Bm, ldb, beta, Cm, ldc);
                return;
            }
            const int64_t slice = kk / parts, rest = kk - slice * parts;  // `parts` equal slices, the remainder as one more
            const double one = 1.0, zero = 0.0;
            if (rocblas_dgemm_strided_batched_64(bh, rocblas_operation_transpose, rocblas_operation_none, m, nn, slice, &one, A, lda, slice, Bm, ldb, slice, &zero,
                                                 scr.X, m, m * nn, parts) != rocblas_status_success) blas_ok = false;
            int np = (int)parts;
            if (rest > 0 && parts < room) {
                gemm(rocblas_operation_transpose, rocblas_operation_none, m, nn, rest, 1.0, A + slice * parts, lda, Bm + slice * parts, ldb, 0.0, scr.X + parts * m * nn, m);
                np++;
            } else if (rest > 0) {
                gemm(rocblas_operation_transpose, rocblas_operation_none, m, nn, rest, 1.0, A + slice * parts, lda, Bm + slice * parts, ldb, 1.0, scr.X + (parts - 1) * m * nn, m);
            }
            hipLaunchKernelGGL(k_sum_parts, g2(m, nn), dim3(T), 0, s, scr.X, m * nn, np, m, nn, alpha, beta, Cm, ldc);
        }
        // Li = inverse of the Cholesky factor of S (m x m, lower triangle read, destroyed), zeros above the diagonal: recursive halves,
        // GEMMs and the in-LDS kernel for blocks of <= 64.  Everything is enqueued; a block that is not positive definite leaves the
        // 1-based position of its first bad pivot in *scr.dinfo (invchol() reads it after the call).
        void invchol_rec(double* S, int64_t lds, double* Li, int64_t ldl, int64_t m, int64_t off) {
            if (m <= TRI_NB) {
                hipLaunchKernelGGL(k_invchol_small, dim3(1), dim3(TRI_NB), 0, s, S, lds, Li, ldl, (int)m, (long long)off, (long long*)scr.dinfo);
                return;
            }
            const int64_t m1 = std::min(m - 1, up64((m + 1) / 2)), m2 = m - m1;
            double *S21 = S + m1, *S22 = S + m1 + m1 * lds, *Li21 = Li + m1, *Li22 = Li + m1 + m1 * ldl;
            double *t1 = scr.tmp2, *t2 = scr.tmp2 + m2 * m1;
            invchol_rec(S, lds, Li, ldl, m1, off);
            gemm(rocblas_operation_none, rocblas_operation_transpose, m2, m1, m1, 1.0, S21, lds, Li, ldl, 0.0, t1, m2);           // L21 = S21 Li11^T
            const double mone = -1.0, one = 1.0;
            if (rocblas_dsyrk_64(bh, rocblas_fill_lower, rocblas_operation_none, m2, m1, &mone, t1, m2, &one, S22, lds) != rocblas_status_success) blas_ok = false;
            gemm(rocblas_operation_none, rocblas_operation_none, m2, m1, m1, 1.0, t1, m2, Li, ldl, 0.0, t2, m2);                    // L21 Li11
            invchol_rec(S22, lds, Li22, ldl, m2, off + m1);
            gemm(rocblas_operation_none, rocblas_operation_none, m2, m1, m2, -1.0, Li22, ldl, t2, m2, 0.0, Li21, ldl);              // Li21 = -Li22 L21 Li11
            hipLaunchKernelGGL(k_fill2d, g2(m1, m2), dim3(T), 0, s, Li + m1 * ldl, ldl, m1, m2, 0.0);
        }
        int64_t invchol(double* S, int64_t lds, double* Li, int64_t ldl, int64_t m) {  // 0, or the 1-based position of the first pivot that is not positive
            if (m <= 0) return 0;
            const int64_t big = INT64_MAX;
            (void)hipMemcpyAsync(scr.dinfo, &big, sizeof(big), hipMemcpyHostToDevice, s);
            (void)hipStreamSynchronize(s);
            invchol_rec(S, lds, Li, ldl, m, 0);
            int64_t info = 0;
            (void)hipMemcpyAsync(&info, scr.dinfo, sizeof(info), hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            return info == INT64_MAX ? 0 : info;
        }

        // ------------------------------------------------------------ setup: the capacity plan, the rocBLAS handle, the buffers
        bool setup() {
            sv.lap_on = log;
            sv.giveup = 0; sv.giveup_text = ""; sv.ok = true;
            sv.block_mark = sv.allocs.size();
            size_t free_b = 0, total_b = 0;
            if (!SWOK(hipMemGetInfo(&free_b, &total_b))) free_b = 0;
            free_b += pool().pooled(sv.dev);  // (handed out again to this very call, or flushed if the sizes differ)
            const bool retry = sv.cap_want > 0;
            const CapacityPlan pl = plan_capacity(n, 0.92 * (double)free_b, sv.cap_want, kn);
            if (retry) sv.cap_want = pl.cap_want;
            if (retry && !pl.fits) return give(FNN_SW_GIVEUP_SETUP, "no factor fits the device memory");
            fac.cap = pl.cap; fac.kmax = pl.kmax; fac.pw = pl.pw; dep.rcap = pl.rcap;
            // (the departed columns' buffers bound how many may stay in the factor: up to this share of it whatever its size, and beyond
            //  that share as long as the buffers keep room for one more block's departures - the rebuild rule of the step loop)
            pol.rfrac_buf = 0.75 * (double)dep.rcap / (double)fac.cap;
            if (log) std::fprintf(stderr, "  [sw] capacity %lld splits (%.2f n), block <= %lld, departed <= %lld; device memory free %.1f GB\n", (long long)fac.cap,
                                  (double)fac.cap / n, (long long)fac.kmax, (long long)dep.rcap, (double)free_b * 1e-9);
            sv.capacity = fac.cap;
            if (rocblas_create_handle(&bh) != rocblas_status_success) { bh = nullptr; return give(FNN_SW_GIVEUP_SETUP, "rocblas_create_handle failed"); }
            rocblas_set_stream(bh, s);
            rocblas_set_pointer_mode(bh, rocblas_pointer_mode_host);
            const double t_alloc0 = sv.wall();
            // (order and byte counts as they are: the pool hands a buffer back to a request of exactly its size)
            const int64_t cap = fac.cap, kmax = fac.kmax, rcap = dep.rcap;
            fac.Ws = TriStore{sv.alloc<double>((size_t)tri_elems(cap, fac.pw)), cap, fac.pw};
            scr.B = sv.alloc<double>((size_t)cap * kmax); scr.Tb = sv.alloc<double>((size_t)cap * kmax); scr.X = sv.alloc<double>((size_t)cap * kmax);
            scr.S = sv.alloc<double>((size_t)kmax * kmax); scr.S0 = sv.alloc<double>((size_t)kmax * kmax); scr.Li = sv.alloc<double>((size_t)kmax * kmax);
            scr.tmp2 = sv.alloc<double>((size_t)(std::max(rcap, kmax) * std::max(rcap, kmax) / 2 + 4096));
            dep.Y = sv.alloc<double>((size_t)cap * rcap);
            dep.CR = sv.alloc<double>((size_t)rcap * rcap); dep.LC = sv.alloc<double>((size_t)rcap * rcap);
            dep.LCs = TriStore{dep.LC, rcap, rcap}; dep.CRb = sv.alloc<double>((size_t)rcap * rcap); dep.CRw = sv.alloc<double>((size_t)rcap * rcap);
            fac.z = sv.alloc<double>((size_t)cap); scr.v = sv.alloc<double>((size_t)cap); fac.xs = sv.alloc<double>((size_t)cap); fac.cK = sv.alloc<double>((size_t)cap);
            dep.lam = sv.alloc<double>((size_t)rcap); fac.gF = sv.alloc<double>((size_t)cap);
            fac.dF = sv.alloc<int2>((size_t)cap); scr.dscr = sv.alloc<int2>((size_t)cap); dep.dlist = sv.alloc<int32_t>((size_t)cap); scr.dlist2 = sv.alloc<int32_t>((size_t)cap);
            scr.wk = sv.alloc<double>((size_t)cap); scr.sk1 = sv.alloc<double>((size_t)cap); scr.sk2 = sv.alloc<double>((size_t)cap); scr.dinfo = sv.alloc<int64_t>(1);
            cand.ccap = std::min<int64_t>(N, std::max<int64_t>(1 << 16, N / 16 + 1024));
            cand.ckey = sv.alloc<double>((size_t)cand.ccap); cand.ckey2 = sv.alloc<double>((size_t)cand.ccap);
            cand.cidx = sv.alloc<int64_t>((size_t)cand.ccap); cand.cidx2 = sv.alloc<int64_t>((size_t)cand.ccap);
            cand.ccount = sv.alloc<unsigned long long>(1);
            if (hipcub::DeviceRadixSort::SortPairsDescending(nullptr, cand.sort_bytes, cand.ckey, cand.ckey2, cand.cidx, cand.cidx2, (int)std::min<int64_t>(cand.ccap, INT32_MAX), 0,
                                                             64, s) != hipSuccess) return give(FNN_SW_GIVEUP_SETUP, "hipcub size query failed");
            cand.sort_tmp = sv.alloc<uint8_t>(cand.sort_bytes + 16);
            if (!sv.ok) return give(FNN_SW_GIVEUP_SETUP, "device allocation of the factor's buffers failed");
            sv.t_alloc_s = sv.wall() - t_alloc0;
            if (log) std::fprintf(stderr, "  [sw] buffers allocated in %.2f s\n", sv.t_alloc_s);
            return true;
        }
        // c = A^T d, the empty mask, the candidates' threshold
        void start() {
            sv.Atx(sv.d, sv.atwd);  // c = A^T d
            (void)hipMemsetAsync(sv.act, 0, (size_t)n * (size_t)ld, s);
            { const Best bb = sv.reduce_best<RD_MAX_UNMASKED>(sv.atwd, nullptr); pol.cmax = bb.k == INT64_MAX ? 0.0 : -bb.v; }
            pol.tol = 1e-12 * (pol.cmax > 0.0 ? pol.cmax : 1.0);
            pol.tol_cap = 1e-10 * (pol.cmax > 0.0 ? pol.cmax : 1.0);
            pol.kmin = std::max<int64_t>(8, n / 32);
            pol.k_limit = fac.kmax;
        }

        // ------------------------------------------------------------ the factor and the departed columns: what a step is made of
        void upload_F(int64_t from, int64_t to) {
            if (to > from) (void)hipMemcpyAsync(fac.dF + from, fac.F.data() + from, sizeof(int2) * (size_t)(to - from), hipMemcpyHostToDevice, s);
        }
        void set_mask(const std::vector<int2>& list, uint8_t v) {  // (through the scratch list: the factor's own list stays as it is)
            if (list.empty()) return;
            (void)hipMemcpyAsync(scr.dscr, list.data(), sizeof(int2) * list.size(), hipMemcpyHostToDevice, s);
            hipLaunchKernelGGL(k_mask, g1((int64_t)list.size()), dim3(T), 0, s, scr.dscr, (int64_t)list.size(), sv.act, ld, v);
            (void)hipStreamSynchronize(s);
        }
        // the weights xw of the factor's splits onto the grid sv.x, zeros elsewhere (enqueued)
        void weights_to_grid() {
            (void)hipMemsetAsync(sv.x, 0, sizeof(double) * (size_t)n * (size_t)ld, s);
            if (fac.f) {
                (void)hipMemcpyAsync(fac.xs, fac.xw.data(), sizeof(double) * (size_t)fac.f, hipMemcpyHostToDevice, s);
                hipLaunchKernelGGL(k_scatter, g1(fac.f), dim3(T), 0, s, fac.dF, fac.f, fac.xs, sv.x, ld);
            }
        }
        // LC = inverse of the Cholesky factor of the Gram matrix CR of the departed columns (lower triangular), from scratch
        bool factor_gram() {
            if (dep.r == 0) return true;
            hipLaunchKernelGGL(k_copy_lower, g2(dep.r, dep.r), dim3(T), 0, s, dep.CR, dep.rcap, dep.CRw, dep.rcap, dep.r);
            return invchol(dep.CRw, dep.rcap, dep.LC, dep.rcap, dep.r) == 0;
        }
        // The core of an append, shared by the factor W (rows for splits that enter) and by LC (rows for columns that depart).
        // phase 1: T = Wi Bc, S = S - T^T T for a lower-triangular inverse factor Wi (f x f); phase 2: rows f .. f + k of Wi
        // from T, the Cholesky factor's inverse Li of S:  [-Li T^T Wi | Li], zeros above.
        void rows_phase1(const TriStore& Wi, int64_t f, const double* Bc, int64_t ldb, int64_t k, double* Tm, int64_t ldt, double* Sm, int64_t lds) {
            if (f == 0) return;
            tri_times(Wi, f, Bc, ldb, k, Tm, ldt);
            tn_splitk(k, k, f, -1.0, Tm, ldt, Tm, ldt, 1.0, Sm, lds);
        }
        void rows_phase2(const TriStore& Wi, int64_t f, const double* Tm, int64_t ldt, const double* Lim, int64_t ldl, int64_t k) {
            if (f > 0) {
                t_times_tri(Tm, ldt, k, Wi, f, scr.X, fac.kmax);  // X = T^T Wi
                for (int64_t q = 0, q0 = 0; q0 < f; q++, q0 += Wi.pw) {  // new rows -Li X, panel by panel
                    const int64_t w = std::min(Wi.pw, f - q0);
                    gemm(rocblas_operation_none, rocblas_operation_none, k, w, k, -1.0, Lim, ldl, scr.X + q0 * fac.kmax, fac.kmax, 0.0, Wi.panel(q) + (f - q0), Wi.ld(q));
                }
            }
            for (int64_t c0 = f; c0 < f + k;) {  // the new columns: zeros above (inside their panel), then Li
                const int64_t q = c0 / Wi.pw, q0 = q * Wi.pw, c1 = std::min(f + k, q0 + Wi.pw);
                if (f > q0)
                    hipLaunchKernelGGL(k_fill2d, g2(f - q0, c1 - c0), dim3(T), 0, s, Wi.at(q0, c0), Wi.ld(q), f - q0, c1 - c0, 0.0);
                // rows [max(f, q0), f + k) of the columns c0 .. c1 (the rows of Li above a panel that starts inside the block are its zeros)
                const int64_t r0 = std::max(f, q0);
                hipLaunchKernelGGL(k_copy2d, g2(f + k - r0, c1 - c0), dim3(T), 0, s, Lim + (c0 - f) * ldl + (r0 - f), ldl, Wi.at(r0, c0), Wi.ld(q), f + k - r0, c1 - c0);
                c0 = c1;
            }
        }
        // the block's Schur complement and multipliers follow the kept splits (append's screening)
        void regather_block(const std::vector<int32_t>& kept, const double* wK) {
            const int64_t kk = (int64_t)kept.size();
            (void)hipMemcpyAsync(scr.dlist2, kept.data(), sizeof(int32_t) * kept.size(), hipMemcpyHostToDevice, s);
            hipLaunchKernelGGL(k_gather_sym, g2(kk, kk), dim3(T), 0, s, scr.S0, fac.kmax, scr.dlist2, kk, scr.S, fac.kmax);
            if (wK) hipLaunchKernelGGL(k_gather_vec, g1(kk), dim3(T), 0, s, wK, scr.dlist2, kk, scr.wk);
            (void)hipStreamSynchronize(s);
        }
        // append the k splits at fac.dF[f .. f + k) with multipliers wK (device, may be null: no screening).  Screening: the block's
        // weights in the joint sub-problem are S^-1 w_K with S the block's Schur complement - known before the rows are formed;
        // splits whose weight would not be positive are dropped here, at half the price and without ever entering the factor.
        // `kept` receives the indices (into the block) of the splits that entered; returns their number, -1 on failure.
        int64_t append(int64_t k, const double* wK, std::vector<int32_t>& kept) {
            const double t0 = log ? sv.wall() : 0.0;
            const int64_t f = fac.f;
            int2* dK = fac.dF + f;
            kept.resize((size_t)k);
            for (int64_t q = 0; q < k; q++) kept[(size_t)q] = (int32_t)q;
            sv.lap(nullptr);
            hipLaunchKernelGGL(k_hblock, g2(k, k), dim3(T), 0, s, dK, k, dK, k, n, scr.S, fac.kmax, 0);
            if (f > 0) hipLaunchKernelGGL(k_hblock, g2(f, k), dim3(T), 0, s, fac.dF, f, dK, k, n, scr.B, fac.cap, 0);
            sv.lap("append.hblock");
            rows_phase1(fac.Ws, f, scr.B, fac.cap, k, scr.Tb, fac.cap, scr.S, fac.kmax);  // T = L^-1 B = L21^T, S = H_KK - L21 L21^T
            sv.lap("append.W*B+syrk");
            hipLaunchKernelGGL(k_copy2d, g2(k, k), dim3(T), 0, s, scr.S, fac.kmax, scr.S0, fac.kmax, k, k);
            const double* wcur = wK;
            std::vector<double> sK;
            bool changed = false;
            for (int round = 0;; round++) {
                const int64_t kk = (int64_t)kept.size();
                const int64_t info = invchol(scr.S, fac.kmax, scr.Li, fac.kmax, kk);  // Li = L22^-1
                if (info > 0) {  // not positive definite at split `info`: the block ends in front of it
                    kept.resize((size_t)(info - 1)); changed = true;
                    if (kept.empty()) return 0;
                    regather_block(kept, wK);
                    if (wK) wcur = scr.wk;
                    continue;
                }
                if (!wK || round >= 12) break;
                // the block's weights in the joint sub-problem: S^-1 w_K = Li^T (Li w_K)
                gemv(rocblas_operation_none, kk, kk, 1.0, scr.Li, fac.kmax, wcur, 0.0, scr.sk1);
                gemv(rocblas_operation_transpose, kk, kk, 1.0, scr.Li, fac.kmax, scr.sk1, 0.0, scr.sk2);
                sK.resize((size_t)kk);
                (void)hipMemcpyAsync(sK.data(), scr.sk2, sizeof(double) * (size_t)kk, hipMemcpyDeviceToHost, s);
                (void)hipStreamSynchronize(s);
                std::vector<int32_t> nk;
                for (int64_t q = 0; q < kk; q++) if (sK[(size_t)q] > 0.0) nk.push_back(kept[(size_t)q]);
                if ((int64_t)nk.size() == kk) break;
                sv.st_screened += kk - (int64_t)nk.size();
                if (nk.empty()) nk.push_back(kept[0]);  // (a single split with a positive multiplier always gets a positive weight)
                kept.swap(nk); changed = true;
                regather_block(kept, wK);
                wcur = scr.wk;
            }
            sv.lap("append.potrf+trtri+screen");
            k = (int64_t)kept.size();
            const double* Tuse = scr.Tb;
            if (changed) {  // T's columns and the split list follow the kept ones (scr.B is free now)
                (void)hipMemcpyAsync(scr.dlist2, kept.data(), sizeof(int32_t) * kept.size(), hipMemcpyHostToDevice, s);
                if (f > 0) { hipLaunchKernelGGL(k_gather_cols, g2(f, k), dim3(T), 0, s, scr.Tb, fac.cap, f, scr.dlist2, k, scr.B, fac.cap); Tuse = scr.B; }
                hipLaunchKernelGGL(k_gather_int2, g1(k), dim3(T), 0, s, dK, scr.dlist2, k, scr.dscr);
                (void)hipMemcpyAsync(dK, scr.dscr, sizeof(int2) * (size_t)k, hipMemcpyDeviceToDevice, s);
                (void)hipStreamSynchronize(s);
            }
            hipLaunchKernelGGL(k_gather, g1(k), dim3(T), 0, s, dK, k, sv.atwd, ld, fac.cK);
            rows_phase2(fac.Ws, f, Tuse, fac.cap, scr.Li, fac.kmax, k);
            if (f > 0) gemv(rocblas_operation_transpose, f, k, -1.0, Tuse, fac.cap, fac.z, 1.0, fac.cK);  // c_K - L21 z
            gemv(rocblas_operation_none, k, k, 1.0, scr.Li, fac.kmax, fac.cK, 0.0, fac.z + f);                // z_K = L22^-1 (c_K - L21 z)
            sv.lap("append.rows");
            if (dep.r > 0) {  // the departed columns grow by the new rows; so does their Gram matrix
                hipLaunchKernelGGL(k_gather_rows_tri, g2(k, dep.r), dim3(T), 0, s, fac.Ws, f, k, dep.dlist, dep.r, dep.Y, fac.cap);
                const double one = 1.0;
                if (rocblas_dsyrk_64(bh, rocblas_fill_lower, rocblas_operation_transpose, dep.r, k, &one, dep.Y + f, fac.cap, &one, dep.CR, dep.rcap) != rocblas_status_success)
                    blas_ok = false;
                if (!factor_gram()) return -1;
                sv.lap("append.gram");
            }
            fac.f = f + k;
            if (log) sv.t_append += sv.wall() - t0;
            return blas_ok ? k : -1;
        }
        void log_departed_positions() const {  // where in the factor did the departed splits sit?
            std::vector<double> pos;
            for (size_t p = 0; p < fac.F.size(); p++) if (dep.dead[p]) pos.push_back((double)p / (double)fac.F.size());
            if (!pos.empty())
                std::fprintf(stderr, "  [sw] rebuild at %zu with %zu departed; their positions: 10%% %.2f 25%% %.2f 50%% %.2f 75%% %.2f\n", fac.F.size(), pos.size(),
                             pos[pos.size() / 10], pos[pos.size() / 4], pos[pos.size() / 2], pos[pos.size() * 3 / 4]);
        }
        // rebuild the factor from H's closed form for the splits that are still in: the compacted list appended in blocks
        bool refactor() {
            const double t0 = log ? sv.wall() : 0.0;
            sv.st_lh_refactor++;
            if (log) log_departed_positions();
            std::vector<int2> gone;
            compact_live(fac.F, fac.xw, fac.cF, dep.dead, dep.deadlist, gone);
            const size_t q = fac.F.size();
            set_mask(gone, 0);  // they may enter again
            fac.f = 0; dep.r = 0;
            if (q == 0) return true;
            upload_F(0, (int64_t)q);
            std::vector<int32_t> kept;
            while (fac.f < (int64_t)q) {
                const int64_t k = std::min<int64_t>({fac.kmax, (int64_t)4096, (int64_t)q - fac.f});
                if (append(k, nullptr, kept) != k) return false;
            }
            (void)hipStreamSynchronize(s);
            if (log) { const double dt = sv.wall() - t0; sv.t_refactor += dt; sv.t_append -= dt; }
            return blas_ok;
        }
        // the splits at the factor positions `idxs` leave: their columns join Y, the Gram matrix and its factor grow
        bool depart(const std::vector<int32_t>& idxs) {
            const double t0 = log ? sv.wall() : 0.0;
            const int64_t nn = (int64_t)idxs.size(), r = dep.r, f = fac.f;
            sv.lap(nullptr);
            (void)hipMemcpyAsync(dep.dlist + r, idxs.data(), sizeof(int32_t) * (size_t)nn, hipMemcpyHostToDevice, s);
            hipLaunchKernelGGL(k_gather_cols_tri, g2(f, nn), dim3(T), 0, s, fac.Ws, f, dep.dlist + r, nn, dep.Y + r * fac.cap, fac.cap);
            // CR[r : r + nn, 0 : r + nn] = YN^T [Y, YN]
            tn_splitk(nn, r + nn, f, 1.0, dep.Y + r * fac.cap, fac.cap, dep.Y, fac.cap, 0.0, dep.CR + r, dep.rcap);
            (void)hipStreamSynchronize(s);  // (idxs may be a temporary)
            sv.lap("depart.gather+gram");
            for (int32_t p : idxs) { dep.dead[(size_t)p] = 1; fac.xw[(size_t)p] = 0.0; dep.deadlist.push_back(p); }
            bool fine = true;
            if (r == 0 || nn > fac.kmax) { dep.r = r + nn; fine = factor_gram(); }
            else {  // border the inverse factor: cross block CR[r:, 0:r]^T, diagonal block CR[r:, r:]
                hipLaunchKernelGGL(k_transpose_small, g2(nn, r), dim3(T), 0, s, dep.CR + r, dep.rcap, nn, r, scr.B, fac.cap);  // (r x nn)
                hipLaunchKernelGGL(k_copy2d, g2(nn, nn), dim3(T), 0, s, dep.CR + r + r * dep.rcap, dep.rcap, scr.S, fac.kmax, nn, nn);
                rows_phase1(dep.LCs, r, scr.B, fac.cap, nn, scr.Tb, fac.cap, scr.S, fac.kmax);
                if (invchol(scr.S, fac.kmax, scr.Li, fac.kmax, nn) != 0) { dep.r = r + nn; fine = factor_gram(); }
                else {
                    rows_phase2(dep.LCs, r, scr.Tb, fac.cap, scr.Li, fac.kmax, nn);
                    dep.r = r + nn;
                }
            }
            sv.lap("depart.gram_factor");
            if (log) sv.t_dead += sv.wall() - t0;
            return fine && blas_ok;
        }
        // Departed splits (factor positions `rev`) come BACK: a split that left is only constrained to zero - its row is still in the
        // factor - so un-constraining it costs the compaction of Y's columns and of the Gram matrix and a fresh Gram factor
        // (r^3, milliseconds), where the route through a rebuild and the candidates re-appends it at f^2 per split.
        bool revive(const std::vector<int32_t>& rev) {
            const double t0 = log ? sv.wall() : 0.0;
            const int64_t r = dep.r, f = fac.f;
            std::vector<int32_t> keepcols, newdead;
            revival_lists(rev, f, dep.dead, dep.deadlist, keepcols, newdead);
            const int64_t rn = (int64_t)keepcols.size();
            sv.st_revived += r - rn;
            if (rn > 0) {
                (void)hipMemcpyAsync(scr.dlist2, keepcols.data(), sizeof(int32_t) * (size_t)rn, hipMemcpyHostToDevice, s);
                hipLaunchKernelGGL(k_gather_sym, g2(rn, rn), dim3(T), 0, s, dep.CR, dep.rcap, scr.dlist2, rn, dep.CRw, dep.rcap);
                hipLaunchKernelGGL(k_copy2d, g2(rn, rn), dim3(T), 0, s, dep.CRw, dep.rcap, dep.CR, dep.rcap, rn, rn);
                // (a kept column's new index is never larger than its old one: chunks of new columns can be written in place)
                for (int64_t c0 = 0; c0 < rn; c0 += fac.kmax) {
                    const int64_t cnt = std::min<int64_t>(fac.kmax, rn - c0);
                    hipLaunchKernelGGL(k_gather_cols, g2(f, cnt), dim3(T), 0, s, dep.Y, fac.cap, f, scr.dlist2 + c0, cnt, scr.B, fac.cap);
                    hipLaunchKernelGGL(k_copy2d, g2(f, cnt), dim3(T), 0, s, scr.B, fac.cap, dep.Y + c0 * fac.cap, fac.cap, f, cnt);
                }
                (void)hipMemcpyAsync(dep.dlist, newdead.data(), sizeof(int32_t) * (size_t)rn, hipMemcpyHostToDevice, s);
                (void)hipStreamSynchronize(s);  // (the host vectors are temporaries)
            }
            dep.deadlist.swap(newdead);
            dep.r = rn;
            const bool fine = factor_gram();
            if (log) sv.t_dead += sv.wall() - t0;
            return fine && blas_ok;
        }
        // minimiser of the sub-problem on the splits that are in: xs = W^T (z - Y (Y^T Y)^-1 Y^T z), copied to `out`
        bool solve(std::vector<double>& out) {
            const double t0 = log ? sv.wall() : 0.0;
            sv.st_solves++;
            const int64_t f = fac.f, r = dep.r;
            out.assign((size_t)f, 0.0);
            if (f == 0) return true;
            const double* vv = fac.z;
            if (r > 0) {
                gemv(rocblas_operation_transpose, f, r, 1.0, dep.Y, fac.cap, fac.z, 0.0, dep.lam);
                gemv(rocblas_operation_none, r, r, 1.0, dep.LC, dep.rcap, dep.lam, 0.0, scr.sk1);       // (Y^T Y)^-1 = LC^T LC
                gemv(rocblas_operation_transpose, r, r, 1.0, dep.LC, dep.rcap, scr.sk1, 0.0, dep.lam);
                (void)hipMemcpyAsync(scr.v, fac.z, sizeof(double) * (size_t)f, hipMemcpyDeviceToDevice, s);
                gemv(rocblas_operation_none, f, r, -1.0, dep.Y, fac.cap, dep.lam, 1.0, scr.v);
                vv = scr.v;
            }
            for (int64_t q = 0, q0 = 0; q0 < f; q++, q0 += fac.Ws.pw) {
                const int64_t w = std::min(fac.Ws.pw, f - q0);
                gemv(rocblas_operation_transpose, f - q0, w, 1.0, fac.Ws.panel(q), fac.Ws.ld(q), vv + q0, 0.0, fac.xs + q0);
            }
            (void)hipMemcpyAsync(out.data(), fac.xs, sizeof(double) * (size_t)f, hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            for (size_t p = 0; p < (size_t)f; p++) if (dep.dead[p]) out[p] = 0.0;
            if (log) sv.t_solve += sv.wall() - t0;
            return blas_ok;
        }
        // the members `out` leave, if the departed columns' buffers have room for them (false: no room, or the departure failed)
        bool depart_counted(const std::vector<int32_t>& out, bool& no_room) {
            no_room = dep.r + (int64_t)out.size() > dep.rcap;
            if (no_room) return false;
            sv.st_dels += (int64_t)out.size();
            for (int32_t p : out) sv.st_dels_new += p >= pol.f_step0 ? 1 : 0;
            return depart(out);
        }
        // every weight that is not positive leaves, until the sub-problem's minimiser is feasible (false: out of room / failure)
        bool settle_all() {
            pol.over_rcap = false;
            for (;;) {
                if (!solve(sbuf)) return false;
                std::vector<int32_t> out;
                for (size_t p = 0; p < sbuf.size(); p++) if (!dep.dead[p] && !(sbuf[p] > 0.0)) out.push_back((int32_t)p);
                if (out.empty()) return true;
                if (!depart_counted(out, pol.over_rcap)) return false;
            }
        }
        // Lawson & Hanson: as far towards the sub-problem's minimiser as feasibility allows; what reaches zero leaves
        bool ratio_loop() {
            std::vector<double> xcur = fac.xw;
            std::vector<int32_t> out;
            for (;;) {
                if (!solve(sbuf)) return false;
                if (ratio_step(xcur, sbuf, dep.dead, out) > 1.0) return true;
                sv.st_ratio_steps++;
                bool no_room = false;
                if (!depart_counted(out, no_room)) { if (no_room) pol.force_rebuild = true; return false; }
            }
        }

        // ------------------------------------------------------------ the steps of the loop
        struct Look {               // what step 1 sees
            int64_t ncand = 0;      // local maxima of the multiplier above the threshold
            double drift = 0.0;     // largest |multiplier| on the splits that are in
            double wdead = 0.0;     // largest multiplier of a departed split
            int64_t dead_wanting = 0;
            std::vector<int32_t> rev;  // departed splits whose multiplier is positive again: they come back with this step (revive)
            double t0 = 0.0;        // (FNN_SW_LOG: start of the selection phase)
        };
        // 1. multipliers: r = c - A^T A x on the grid; the entries at the factor's splits go to the host; the candidates
        Look look() {
            Look lk;
            double t0 = log ? sv.wall() : 0.0;
            weights_to_grid();
            sv.Ab(sv.x, sv.y);
            sv.Atx(sv.y, sv.r);
            std::vector<double> gF((size_t)fac.f);
            if (fac.f) {
                hipLaunchKernelGGL(k_gather, g1(fac.f), dim3(T), 0, s, fac.dF, fac.f, sv.r, ld, fac.gF);
                (void)hipMemcpyAsync(gF.data(), fac.gF, sizeof(double) * (size_t)fac.f, hipMemcpyDeviceToHost, s);
            }
            sv.vec<OP_R_INIT>(sv.r, nullptr, sv.atwd, nullptr);  // r = masked ? 0 : c - r
            if (log) sv.t_ops += sv.wall() - t0;
            lk.t0 = log ? sv.wall() : 0.0;
            (void)hipMemsetAsync(cand.ccount, 0, sizeof(unsigned long long), s);
            hipLaunchKernelGGL(k_candidates, sv.grid2, dim3(T), 0, s, sv.r, sv.act, n, ld, pol.tol, kn.nms, cand.ckey, cand.cidx, cand.ccount, (unsigned long long)cand.ccap);
            unsigned long long ncand64 = 0;
            (void)hipMemcpyAsync(&ncand64, cand.ccount, sizeof(ncand64), hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            lk.ncand = (int64_t)std::min<unsigned long long>(ncand64, (unsigned long long)cand.ccap);
            // (gF holds A^T A x at the factor's splits: c - gF is the multiplier of a split that left, the drift at one that is in)
            for (size_t p = 0; p < (size_t)fac.f; p++) {
                const double g = fac.cF[p] - gF[p];
                if (dep.dead[p]) {
                    lk.wdead = std::max(lk.wdead, g); lk.dead_wanting += g > pol.tol ? 1 : 0;
                    // (tried: returns only once the factor holds 8192 splits - 82.2 s instead of 73.0 s at 32768 taxa)
                    if (g > pol.tol && kn.revive != 0 && !pol.revive_blocked) lk.rev.push_back((int32_t)p);
                } else lk.drift = std::max(lk.drift, std::fabs(g));
            }
            sv.st_dead_wanting += lk.dead_wanting;
            if (kn.revive == 2 && lk.ncand != 0) lk.rev.clear();
            return lk;
        }
        // 2. the block size ...
        int64_t block_size(const Look& lk) const {
            const int64_t nlive = fac.f - dep.r;
            int64_t k = (int64_t)std::min<double>((double)fac.kmax, std::max<double>((double)pol.kmin, kn.kfrac * (double)std::max<int64_t>(nlive, 1)));
            k = std::max<int64_t>(1, std::min<int64_t>({k, lk.ncand, pol.k_limit}));
            if (lk.ncand != 0 && dep.r == 0 && fac.f + k > fac.cap && fac.f < fac.cap) k = fac.cap - fac.f;  // (nothing to rebuild away: fill the factor to the brim first)
            return k;
        }
        // ... and the rebuild rule: a split that left wants back in, the factor has drifted or is full of departed splits
        bool rebuild_due(const Look& lk, int64_t k) const {
            const bool no_cand = lk.ncand == 0;
            // (the drift of the gradient on the splits that are in: half of what the solver's own Kuhn-Tucker check allows at the end)
            // (departed splits in the factor: each costs every append 4 k f flops and every departure its share of the Gram matrix; a
            //  rebuild costs 2/3 f^3 - FNN_SW_RFRAC is the share of the factor at which the rebuild is taken)
            const double r_limit = std::min(kn.rfrac * (double)fac.f, std::max(pol.rfrac_buf * (double)fac.f, (double)dep.rcap - 1.5 * (double)k));
            return (no_cand && lk.rev.empty() && (lk.wdead > pol.tol || (lk.drift > 5e-10 * pol.cmax && !pol.fresh))) ||
                   (!no_cand && (fac.f + k > fac.cap || (double)(dep.r - (int64_t)lk.rev.size()) > r_limit || (pol.force_rebuild && dep.r > 0)));
        }
        // rebuild the factor, solve, look again
        void rebuild(const Look& lk) {
            pol.force_rebuild = false;
            if (lk.ncand != 0 && dep.r == 0) { give(FNN_SW_GIVEUP_CAPACITY, "the free set outgrew the dense factor"); return; }  // the caller decides about the reference's route
            if (!refactor()) { give(FNN_SW_GIVEUP_NUMERIC, "rebuild of the factor failed"); return; }
            if (!settle_all()) { give(pol.over_rcap ? FNN_SW_GIVEUP_DEPARTED : FNN_SW_GIVEUP_NUMERIC, pol.over_rcap ? "departed splits outgrew their buffers after a rebuild" : "sub-problem solve failed"); return; }
            fac.xw = sbuf; pol.phi = objective(fac.xw, fac.cF, dep.dead); pol.fresh = true;
        }
        // 3. no candidate left, nothing to bring back.  Splits that were set aside (numerically dependent on the factor at the time, or
        // no measurable descent) are still masked: before the method may call this the optimum they get one more look against the
        // current factor.
        void no_candidate_left() {
            if (!pol.banned.empty() && !pol.banned_rechecked) { set_mask(pol.banned, 0); pol.banned.clear(); pol.banned_rechecked = true; return; }
            sv.n_set_aside = (int64_t)pol.banned.size();
            done = true;
        }
        // The state a block that does not descend is taken back to (the appended rows are simply dropped)
        struct Snapshot {
            int64_t f0 = 0, r0 = 0;
            std::vector<uint8_t> dead0;
            std::vector<double> x0;
            std::vector<int32_t> deadlist0;
            void save(BlockMethod& m) {  // (the Gram matrix of the departed columns goes to its copy CRb)
                f0 = m.fac.f; r0 = m.dep.r;
                dead0 = m.dep.dead; x0 = m.fac.xw; deadlist0 = m.dep.deadlist;
                if (r0 > 0) hipLaunchKernelGGL(k_copy2d, g2(r0, r0), dim3(T), 0, m.s, m.dep.CR, m.dep.rcap, m.dep.CRb, m.dep.rcap, r0, r0);
            }
            bool restore(BlockMethod& m, bool revived) const {  // false: the Gram factor of the departed columns failed
                Factor& fac = m.fac; Departed& dep = m.dep;
                if (fac.f > f0) hipLaunchKernelGGL(k_mask, g1(fac.f - f0), dim3(T), 0, m.s, fac.dF + f0, fac.f - f0, m.sv.act, m.ld, (uint8_t)0);
                fac.f = f0; dep.r = r0;
                fac.F.resize((size_t)f0); dep.dead = dead0; fac.xw = x0; dep.deadlist = deadlist0; fac.cF.resize((size_t)f0);
                if (r0 == 0) return true;
                hipLaunchKernelGGL(k_copy2d, g2(r0, r0), dim3(T), 0, m.s, dep.CRb, dep.rcap, dep.CR, dep.rcap, r0, r0);
                (void)hipMemcpyAsync(dep.dlist, dep.deadlist.data(), sizeof(int32_t) * (size_t)r0, hipMemcpyHostToDevice, m.s);
                // (departed splits had come back with this step: Y's columns were compacted - fetch them from the factor again)
                if (revived) hipLaunchKernelGGL(k_gather_cols_tri, g2(f0, r0), dim3(T), 0, m.s, fac.Ws, f0, dep.dlist, r0, dep.Y, fac.cap);
                (void)hipStreamSynchronize(m.s);
                return m.factor_gram();
            }
        };
        struct Block { int64_t kin = 0; int2 entered = make_int2(-1, -1); bool proceed = true; };
        // 4. the block enters: the k largest local maxima of the multiplier (none: a step that only brings departed splits back).
        // proceed = false: the step ends here (a give-up, or the first split was set aside and nothing comes back)
        Block enter(const Look& lk, int64_t k, int64_t f0) {
            Block blk;
            if (lk.ncand == 0) return blk;
            blk.proceed = false;
            if (hipcub::DeviceRadixSort::SortPairsDescending(cand.sort_tmp, cand.sort_bytes, cand.ckey, cand.ckey2, cand.cidx, cand.cidx2, (int)lk.ncand, 0, 64, s) != hipSuccess) {
                give(FNN_SW_GIVEUP_NUMERIC, "candidate sort failed"); return blk;
            }
            hipLaunchKernelGGL(k_idx_to_split, g1(k), dim3(T), 0, s, cand.cidx2, k, ld, fac.dF + fac.f);
            fac.F.resize((size_t)(fac.f + k));
            (void)hipMemcpyAsync(fac.F.data() + fac.f, fac.dF + fac.f, sizeof(int2) * (size_t)k, hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            // (tried: returns only for multipliers that would have made the block - fewer returns, but more one-split solves: 78.0 s
            //  instead of 74.4 s at 32768 taxa)
            if (log) sv.t_sel += sv.wall() - lk.t0;
            // ---- it enters, the weights that are not positive leave, the objective decides
            const int2 first = fac.F[(size_t)f0];
            std::vector<int32_t> kept;
            blk.kin = append(k, cand.ckey2, kept);
            if (blk.kin < 0) { give(FNN_SW_GIVEUP_NUMERIC, "append failed (BLAS / Cholesky)"); return blk; }
            if (blk.kin == 0) {  // the first split is numerically dependent on the factor: set it aside until progress is made
                fac.F.resize((size_t)f0);
                pol.banned.push_back(first); set_mask({first}, 1);
                blk.proceed = !lk.rev.empty();
                return blk;
            }
            const int64_t kin = blk.kin;
            for (int64_t q = 0; q < kin; q++) fac.F[(size_t)(f0 + q)] = fac.F[(size_t)(f0 + kept[(size_t)q])];
            fac.F.resize((size_t)(f0 + kin));
            blk.entered = fac.F[(size_t)f0];
            hipLaunchKernelGGL(k_mask, g1(kin), dim3(T), 0, s, fac.dF + f0, kin, sv.act, ld, (uint8_t)1);
            sv.st_adds += kin;
            fac.xw.resize((size_t)fac.f, 0.0); dep.dead.resize((size_t)fac.f, 0); fac.cF.resize((size_t)fac.f);
            hipLaunchKernelGGL(k_gather, g1(kin), dim3(T), 0, s, fac.dF + f0, kin, sv.atwd, ld, fac.xs);
            (void)hipMemcpyAsync(fac.cF.data() + f0, fac.xs, sizeof(double) * (size_t)kin, hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            blk.proceed = true;
            return blk;
        }
        // 5. the two ways to feasibility: all weights that are not positive leave at once, or Lawson & Hanson's ratio step
        bool make_feasible() {
            if (pol.ratio_mode) return ratio_loop();
            const bool feasible = settle_all();
            if (!feasible && pol.over_rcap) pol.force_rebuild = true;
            return feasible;
        }
        // The candidates' threshold rises to the block's largest multiplier - the noise floor of this problem - if that is below tol_cap,
        // or if `forced`.  false: it is above, and the threshold stays.  (stalled: the steps without measurable descent, 0: a single split)
        bool noise_floor(int stalled, bool forced) {
            double wtop = 0.0;
            (void)hipMemcpyAsync(&wtop, cand.ckey2, sizeof(double), hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            if (!(wtop <= pol.tol_cap || forced)) return false;
            const double rel = wtop / (pol.cmax > 0.0 ? pol.cmax : 1.0);
            if (stalled) {
                if (log || wtop > pol.tol_cap) std::fprintf(stderr, "  [sw] noise floor after %d steps without measurable descent: candidates' threshold %.3g -> %.3g (%.3g max|A^T d|)\n",
                                                            stalled, pol.tol, wtop, rel);
            } else if (log) std::fprintf(stderr, "  [sw] noise floor: candidates' threshold %.3g -> %.3g (%.3g max|A^T d|)\n", pol.tol, wtop, rel);
            pol.tol = std::max(pol.tol, wtop);
            return true;
        }
        // 6. no descent: the factor as it was before this block, and what the next step does differently
        void take_back(const Look& lk, const Block& blk, const Snapshot& snap, bool revived, double phi_new) {
            const int64_t kin = blk.kin;
            sv.st_rejects++;
            if (log) std::fprintf(stderr, "  [sw] step %lld: block of %lld (+%lld departed splits back) at |F| = %lld taken back (%.17g vs %.17g)%s\n", (long long)sv.st_lh_steps,
                                  (long long)kin, (long long)lk.rev.size(), (long long)(snap.f0 - snap.r0), phi_new, pol.phi, pol.ratio_mode ? " [ratio step]" : "");
            if (!snap.restore(*this, revived)) { give(FNN_SW_GIVEUP_NUMERIC, "Gram factor of the departed columns failed"); return; }
            if (revived) pol.revive_blocked = true;    // (no returns again before a step has moved)
            if (revived && kin == 0) return;           // (nothing had entered: only the returns are taken back)
            // the same block once more with Lawson & Hanson's step, which cannot ascend; if that made no progress either (rounding
            // noise at this level): a quarter of the block, and a single split that does not move is set aside
            if (!pol.ratio_mode) { pol.ratio_mode = true; pol.k_limit = kin; return; }
            // One split, the step that cannot ascend, and still no descent: the objective no longer resolves what this
            // multiplier is worth.  If the block's largest multiplier is below 1e-10 max|A^T d| (a tenth of what the
            // Kuhn-Tucker certificate of the tests allows), that level IS the noise floor of this problem - tree-like
            // distances at 32768 taxa: objective 9e10, changes in its 14th digit, thousands of such candidates, each
            // worth a step - and becomes the candidates' threshold; a larger one is set aside until a step moves.
            if (kin == 1 && !noise_floor(0, false)) { pol.banned.push_back(blk.entered); set_mask({blk.entered}, 1); }
            pol.k_limit = std::max<int64_t>(1, kin / 4);
        }
        // 7. the step is taken
        void accept(const Look& lk, const Block& blk, double phi_new, double phi_eps) {
            const bool moved = pol.phi - phi_new > phi_eps;  // (a descent in the last digits is not progress)
            pol.phi = phi_new; fac.xw = sbuf; pol.fresh = false;
            pol.stall = moved ? 0 : pol.stall + 1;
            // Eight steps that the objective cannot tell apart: the candidates' multipliers are at the noise floor of this
            // problem (tree-like distances at 32768 taxa: objective 9e10, thousands of candidates around 1e-11 max|A^T d|,
            // each good for a step in the 14th digit).  Their level becomes the candidates' threshold, as long as it is
            // below 1e-10 max|A^T d| (a tenth of what the tests' Kuhn-Tucker certificate allows); above that only after
            // 200 such steps, with a line in the log, so that the method ends.
            if (pol.stall >= 8 && noise_floor(pol.stall, pol.stall >= 200)) pol.stall = 0;
            pol.k_limit = pol.k_limit > fac.kmax / 2 ? fac.kmax : 2 * pol.k_limit;
            // near the end (few candidates, each displacing one split) the guaranteed step stays on.  (Tried, round 4: the guaranteed step
            // only for the retry of a block that did not descend, and for eight steps after three such blocks in a row - 75.6 s instead
            // of 73.0 s at 32768 taxa, 13.9 s instead of 13.4 s at 16384: the method's path is sensitive to such rules, +-10 %.)
            pol.ratio_mode = pol.ratio_mode && lk.ncand <= 2 * pol.kmin;
            if (moved) pol.revive_blocked = false;
            if (moved) pol.banned_rechecked = false;
            if (moved && !pol.banned.empty()) { set_mask(pol.banned, 0); pol.banned.clear(); }  // progress: the splits set aside may be looked at again
            if (log && (sv.st_lh_steps % 10 == 0 || sv.st_lh_steps < 5))
                std::fprintf(stderr, "  [sw] step %lld: |F| = %lld (+%lld departed in the factor) candidates %lld block %lld solves %lld objective %.12g | ops %.2f sel %.2f "
                             "append %.2f solve %.2f depart %.2f refactor %.2f s\n", (long long)sv.st_lh_steps, (long long)(fac.f - dep.r), (long long)dep.r, (long long)lk.ncand,
                             (long long)blk.kin, (long long)sv.st_solves, pol.phi, sv.t_ops, sv.t_sel, sv.t_append, sv.t_solve, sv.t_dead, sv.t_refactor);
        }
        void log_summary() const {
            std::fprintf(stderr, "  [sw] %s: %lld steps, %lld solves, %lld entered (%lld screened out before), %lld left, %lld taken back, %lld ratio steps, %lld factorisations; |F| = %lld | ops %.2f "
                         "sel %.2f append %.2f solve %.2f depart %.2f refactor %.2f s\n", good ? "done" : "gave up", (long long)sv.st_lh_steps, (long long)sv.st_solves,
                         (long long)sv.st_adds, (long long)sv.st_screened, (long long)sv.st_dels, (long long)sv.st_rejects, (long long)sv.st_ratio_steps, (long long)sv.st_lh_refactor, (long long)(fac.f - dep.r),
                         sv.t_ops, sv.t_sel, sv.t_append, sv.t_solve, sv.t_dead, sv.t_refactor);
            std::fprintf(stderr, "  [sw]   GEMM work through gemm(): %.3e flop; departed splits with a positive multiplier, summed over the steps: %lld; brought back: %lld; "
                         "departures of splits in the step they entered: %lld\n", sv.gemm_flops, (long long)sv.st_dead_wanting, (long long)sv.st_revived, (long long)sv.st_dels_new);
            for (const auto& kv : sv.tsub) std::fprintf(stderr, "  [sw]   %-28s %8.3f s\n", kv.first.c_str(), kv.second);
        }

        // true: the optimum's weights are on the grid sv.x; false: sv.giveup says why not
        bool run() {
            if (!setup()) return false;
            start();
            Snapshot snap;
            const int64_t max_outer = 40 * (int64_t)n + 1000;
            while (good && !done && sv.st_lh_steps < max_outer) {  // (st_lh_steps counts over the attempts of a call, as the other counters do)
                sv.st_lh_steps++;
                pol.f_step0 = INT64_MAX;
                const Look lk = look();                                                   // 1. multipliers and candidates
                const int64_t k = block_size(lk);                                         // 2. the block size; the rebuild where it is due
                if (rebuild_due(lk, k)) { rebuild(lk); continue; }
                if (lk.ncand == 0 && lk.rev.empty()) { no_candidate_left(); continue; }   // 3. no candidate left
                snap.save(*this);
                pol.f_step0 = snap.f0;
                const Block blk = enter(lk, k, snap.f0);                                  // 4. the block enters
                if (!blk.proceed) continue;
                const bool revived = !lk.rev.empty();
                if (revived && !revive(lk.rev)) { give(FNN_SW_GIVEUP_NUMERIC, "Gram factor of the departed columns failed"); continue; }
                const bool feasible = make_feasible();                                    // 5. to feasibility
                if (!blas_ok) { give(FNN_SW_GIVEUP_NUMERIC, "a BLAS call failed"); continue; }
                sv.f_peak = std::max(sv.f_peak, fac.f);
                const double phi_new = feasible ? objective(sbuf, fac.cF, dep.dead) : INFINITY;
                // Lawson & Hanson's step moves along the segment to the minimiser of a convex quadratic: it cannot ascend, so an
                // "ascent" in the objective's last digits is rounding and the step is taken; the other step has to descend.
                const double phi_eps = 1e-13 * std::fabs(pol.phi);
                if (!(pol.ratio_mode ? phi_new < pol.phi + phi_eps : phi_new < pol.phi)) take_back(lk, blk, snap, revived, phi_new);  // 6. no descent
                else accept(lk, blk, phi_new, phi_eps);                                   // 7. acceptance
            }
            if (!done && good) give(FNN_SW_GIVEUP_STEPS, "step limit reached");
            sv.final_tol_rel = pol.tol / (pol.cmax > 0.0 ? pol.cmax : 1.0);
            sv.have_atwd = true;
            if (good) {  // the optimum on the grid
                weights_to_grid();
                (void)hipStreamSynchronize(s);
            }
            if (log) log_summary();
            return good;
        }
    };

    // runActiveConjugate (:366-557)
    void active_conjugate() {
        hipLaunchKernelGGL(k_unconstrained, dim3((n + T - 1) / T, n), dim3(T), 0, s, d, x, n, ld);
        if (reduce_sum<RD_COUNT_NEG>(x, nullptr) == 0.0) return;
        (void)hipMemsetAsync(act, 0, (size_t)n * (size_t)ld, s);
        hipLaunchKernelGGL(k_fill, dim3((unsigned)((n * ld + T - 1) / T)), dim3(T), 0, s, old_x, (int64_t)n * ld, 1.0);  // Arrays.fill(old_x, 1.0) (:383)
        Atx(d, atwd);
        bool first_pass = true;
        for (;;) {
            st_outer++;
            for (;;) {
                if (!first_pass) cg();
                first_pass = false;
                if (contract_worst()) cg();
                const Best mr = reduce_best<RD_MIN_RATIO>(x, old_x);
                if (mr.k == INT64_MAX) break;  // feasible
                vec<OP_MOVE_OLD>(x, old_x, nullptr, nullptr, mr.v);
                const uint8_t one = 1;
                const double zero = 0.0;
                (void)hipMemcpyAsync(act + mr.k, &one, 1, hipMemcpyHostToDevice, s);
                (void)hipMemcpyAsync(x + mr.k, &zero, sizeof(double), hipMemcpyHostToDevice, s);
                (void)hipStreamSynchronize(s);
            }
            Ab(x, y);
            Atx(y, r);
            vec<OP_GRAD>(r, nullptr, atwd, nullptr);
            const Best mg = reduce_best<RD_MIN_ACTIVE_GRAD>(r, nullptr);
            if (mg.k == INT64_MAX || mg.v > -0.0000001) break;
            const uint8_t zero8 = 0;
            (void)hipMemcpyAsync(act + mg.k, &zero8, 1, hipMemcpyHostToDevice, s);
            (void)hipStreamSynchronize(s);
        }
    }
};

}  // namespace fnnsw

// The caller's statistics.  done == nullptr: the block method gave up (written before the call fails or the reference's route
// starts) - what it counted, zeros elsewhere; else the call's normal end.
struct Outcome { int route; int64_t npos; bool certified; double viol, t_solve_s; };
static void fill_stats(fnn_sw_stats* stats, const fnnsw::Solver& S, const Outcome* done) {
    if (!stats) return;
    std::memset(stats, 0, sizeof(*stats));
    const bool from_below = done && done->route == FNN_SW_ROUTE_FROM_BELOW;
    stats->giveup_reason = S.giveup; stats->capacity = S.capacity; stats->free_set_peak = S.f_peak;
    stats->outer_iterations = (!done || from_below) ? S.st_lh_steps : S.st_outer;
    stats->entered = S.st_adds; stats->screened_out = S.st_screened; stats->departed = S.st_dels;
    if (!done) return;
    stats->cg_calls = S.st_cg;
    stats->cg_iterations = S.st_it;
    stats->reserved[0] = from_below ? 1 : 0;        // method: 1 = from below (block active-set, dense factor), 0 = the reference's (or the closed form)
    stats->reserved[1] = S.st_lh_refactor;
    stats->reserved[2] = S.st_solves;               // sub-problems solved (from below)
    stats->t_solve_s = done->t_solve_s;
    stats->nsplits = done->npos;                    // weights above the threshold (FastNN.java:455: 1e-6; the sparse call: its own)
    stats->route = done->route;
    stats->certified = done->certified ? 1 : 0;
    stats->kkt_violation = done->viol;
    stats->final_threshold_rel = from_below ? S.final_tol_rel : 0.0;
    stats->n_set_aside = from_below ? S.n_set_aside : 0;
    stats->t_alloc_s = S.t_alloc_s;
}

// weights_out != nullptr: all n (n - 1) / 2 weights; else the weights above `thr` as (index, weight) pairs in index order
static int32_t split_weights_impl(const double* D, int32_t n, int64_t ldD, const int32_t* ordering, int32_t device, double* weights_out,
                                  double thr, int64_t* idx_out, double* w_out, int64_t cap_out, int64_t* count_out, fnn_sw_stats* stats) {
    using namespace fnnsw;
    const Knobs kn = Knobs::from_env();  // every FNN_SW_* switch of this file, read once per call
    if (!D || !ordering || n < 2 || ldD < n || (!weights_out && (!idx_out || !w_out || !count_out || cap_out < 0)))
        return fnn::fail(FNN_EINVAL, "fnn_split_weights_f64: bad arguments");
    {
        std::vector<char> seen((size_t)n + 1, 0);
        for (int i = 1; i <= n; i++) {
            if (ordering[i] < 1 || ordering[i] > n || seen[(size_t)ordering[i]]) return fnn::fail(FNN_EINVAL, "fnn_split_weights_f64: ordering is not a permutation of 1..n");
            seen[(size_t)ordering[i]] = 1;
        }
    }
    int cnt = 0;
    if (!SWOK(hipGetDeviceCount(&cnt)) || cnt <= 0) return fnn::fail(FNN_EHIP, "no HIP device available");
    if (device < 0 || device >= cnt || !SWOK(hipSetDevice(device))) return fnn::fail(FNN_EINVAL, "device ordinal out of range");
    struct Events {  // (destroyed on every exit path)
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    Solver S;
    S.dev = device;
    S.n = n;
    S.ld = ((int64_t)n + 31) / 32 * 32 + 32;
    if (!SWOK(hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking))) return fnn::fail(FNN_EHIP, "hipStreamCreate failed");
    const size_t NN = (size_t)n * (size_t)S.ld;
    // (w, p, old_x belong to the reference's method only and are allocated when it runs)
    S.d = S.alloc<double>(NN); S.x = S.alloc<double>(NN); S.r = S.alloc<double>(NN);
    S.y = S.alloc<double>(NN); S.atwd = S.alloc<double>(NN);
    S.P = S.alloc<double>(NN); S.Pt = S.alloc<double>(NN); S.rs = S.alloc<double>((size_t)n + 8);
    S.act = S.alloc<uint8_t>(NN);
    S.Dm = S.alloc<double>((size_t)n * (size_t)n);
    S.ord = S.alloc<int32_t>((size_t)n + 1);
    S.live = S.alloc<double>((size_t)n * (n - 1) / 2);
    S.grid2 = dim3((unsigned)((n + T - 1) / T), (unsigned)n);
    S.gred = dim3((unsigned)((n + T - 1) / T), (unsigned)(n < 256 ? n : 256));
    S.partial = S.alloc<double>(4 * (size_t)S.gred.x * S.gred.y);
    S.sc = S.alloc<double>(SC_WORDS);
    S.bpartial = S.alloc<Best>((size_t)S.gred.x * S.gred.y);
    if (!S.ok) return fnn::fail(FNN_ENOMEM, "fnn_split_weights_f64: device allocation failed");
    for (double* v : {S.d, S.x, S.r, S.y, S.atwd, S.P, S.Pt}) (void)hipMemsetAsync(v, 0, sizeof(double) * NN, S.s);
    if (!SWOK(hipMemcpy2DAsync(S.Dm, sizeof(double) * (size_t)n, D, sizeof(double) * (size_t)ldD, sizeof(double) * (size_t)n, (size_t)n,
                               hipMemcpyHostToDevice, S.s)) ||
        !SWOK(hipMemcpyAsync(S.ord, ordering, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, S.s)) ||
        !SWOK(hipStreamSynchronize(S.s)))
        return fnn::fail(FNN_EHIP, "fnn_split_weights_f64: upload failed");
    if (!SWOK(hipEventCreate(&ev.e0)) || !SWOK(hipEventCreate(&ev.e1))) return fnn::fail(FNN_EHIP, "fnn_split_weights_f64: hipEventCreate failed");
    (void)hipEventRecord(ev.e0, S.s);
    hipLaunchKernelGGL(k_reorder, dim3((unsigned)((n + T - 1) / T), (unsigned)n), dim3(T), 0, S.s, S.Dm, (int64_t)n, S.ord, S.d, n, S.ld);
    S.release(S.Dm);  // (the raw copy has served: its n^2 doubles go back to the pool before the factor is sized)
    S.Dm = nullptr;
    // A NaN or an infinity among the distances makes every comparison below false: the closed form would be "feasible" and NaN
    // weights would go back with FNN_OK.  Refuse them before any route is chosen.
    if (S.reduce_sum<RD_COUNT_NONFINITE>(S.d, nullptr) != 0.0)
        return fnn::fail(FNN_EINVAL, "fnn_split_weights_f64: the distances contain a NaN or an infinity");
    // the closed form if it is feasible; else from below (block active-set method, exact sub-problems); the reference's own
    // method (from above, conjugate gradients) where the free set is too large for a dense factor AND that route is affordable
    int route = FNN_SW_ROUTE_CLOSED_FORM;
    hipLaunchKernelGGL(k_unconstrained, dim3((unsigned)((n + T - 1) / T), (unsigned)n), dim3(T), 0, S.s, S.d, S.x, n, S.ld);
    if (S.reduce_sum<RD_COUNT_NEG>(S.x, nullptr) != 0.0) {
        const bool want_reference = kn.reference_method;
        // The block method's factor is sized for the common case (random or tree-like distances: 2.4 n ... 3.8 n positive splits) so
        // that small problems do not pay for a 100-GB allocation; distances whose optimum has more positive splits (nearly
        // circular metrics: measured 19.5 n at 1024 taxa with 1 % noise) outgrow it: try again with four times the capacity, up to
        // what device memory holds (~150 000 splits, whatever n) or all n (n - 1) / 2 splits.
        bool from_below = false;
        if (!want_reference) {
            const int64_t Nall = (int64_t)n * (n - 1) / 2;
            for (int attempt = 0; attempt < 6; attempt++) {
                {   // (its rocBLAS handle and the handle's workspace are gone before the free memory is read for another attempt)
                    Solver::BlockMethod attempt_(S, kn);
                    from_below = attempt_.run();
                }
                if (from_below || S.giveup != FNN_SW_GIVEUP_CAPACITY || S.capacity >= Nall || kn.cap_set) break;
                const int64_t prev = S.capacity;
                S.release_block_buffers();
                S.cap_want = std::min<int64_t>(Nall, 4 * prev);
                size_t fb = 0, tb = 0;
                if (hipMemGetInfo(&fb, &tb) != hipSuccess) break;
                fb += pool().pooled(device);
                // (the largest factor that can fit at all: cap^2 * 8 B * 9/16 for the factor alone)
                const int64_t hard = (int64_t)std::sqrt(0.9 * (double)fb / (8.0 * 0.62 * 1.7));
                if (S.cap_want > hard) S.cap_want = hard;
                if (S.cap_want < prev + prev / 4) { S.cap_want = 0; break; }  // no meaningful growth left: the give-up stands
                std::fprintf(stderr, "fnn_split_weights_f64: the free set outgrew the factor's capacity of %lld splits at n = %d; once more with %lld\n",
                             (long long)prev, n, (long long)S.cap_want);
            }
        }
        route = from_below ? FNN_SW_ROUTE_FROM_BELOW : FNN_SW_ROUTE_REFERENCE;
        if (!from_below) {
            if (!want_reference) {
                // The block method gave up.  Say so, always: the route that follows is the reference's own - correct, but
                // O(n^2) work per conjugate-gradient iteration and thousands of iterations on large problems.
                // (the default of FNN_SW_REFERENCE_MAX_N, 1024, measured: a 1024-taxon nearly circular input takes 80 s on that route, 2048 taxa more than 5 min)
                const bool allow = kn.allow_reference || n <= kn.reference_max_n;
                std::fprintf(stderr, "fnn_split_weights_f64: the block active-set method gave up at n = %d (%s; capacity %lld splits, free set peaked at %lld): %s\n",
                             n, S.giveup_text, (long long)S.capacity, (long long)S.f_peak,
                             kn.no_reference ? "FNN_SW_NO_REFERENCE_ROUTE is set"
                             : allow ? "taking the reference's active-set / conjugate-gradient route"
                                     : "the reference's conjugate-gradient route is not taken automatically above FNN_SW_REFERENCE_MAX_N taxa");
                fill_stats(stats, S, nullptr);
                if (kn.no_reference || !allow) {
                    const bool cap = S.giveup == FNN_SW_GIVEUP_CAPACITY || S.giveup == FNN_SW_GIVEUP_DEPARTED || S.giveup == FNN_SW_GIVEUP_SETUP;
                    return fnn::fail(cap ? FNN_ECAPACITY : FNN_EHIP,
                                     std::string("fnn_split_weights_f64: the block active-set method gave up (") + S.giveup_text + "); the optimum of these distances has more "
                                     "positive splits than the dense factor holds (" + std::to_string((long long)S.capacity) + "), and the reference's conjugate-gradient route "
                                     "is not taken automatically at this size (FNN_SW_ALLOW_REFERENCE_ROUTE=1 takes it)");
                }
            }
            S.release_block_buffers();
            S.w = S.alloc<double>(NN); S.p = S.alloc<double>(NN); S.old_x = S.alloc<double>(NN);
            if (!S.ok) return fnn::fail(FNN_ENOMEM, "fnn_split_weights_f64: device allocation failed");
            for (double* v : {S.w, S.p, S.old_x}) (void)hipMemsetAsync(v, 0, sizeof(double) * NN, S.s);
            S.st_lh_steps = 0; S.st_solves = 0;
            S.active_conjugate();
            S.have_atwd = true;
        }
    }
    if (kn.fault_perturb) hipLaunchKernelGGL(k_fault_perturb, dim3(1), dim3(1), 0, S.s, S.x, n, S.ld);
    hipLaunchKernelGGL(k_to_live, S.grid2, dim3(T), 0, S.s, S.x, S.live, n, S.ld);
    (void)hipEventRecord(ev.e1, S.s);
    // The solver's own Kuhn-Tucker check of what it returns: g = A^T (A x - d) from the implicit operators, which share
    // nothing with the factor the block method solved with (outside the timed span: ~0.15 s at 32768 taxa)
    if (!S.have_atwd) S.Atx(S.d, S.atwd);
    S.Ab(S.x, S.y);
    hipLaunchKernelGGL(k_sub, S.grid2, dim3(T), 0, S.s, S.y, S.d, n, S.ld);
    S.Atx(S.y, S.r);
    hipLaunchKernelGGL(k_kkt, S.gred, dim3(T), 0, S.s, S.x, S.r, S.atwd, n, S.ld, S.partial);
    std::vector<double> kp(4 * (size_t)S.gred.x * S.gred.y);
    (void)hipMemcpyAsync(kp.data(), S.partial, sizeof(double) * kp.size(), hipMemcpyDeviceToHost, S.s);
    hipError_t e = hipStreamSynchronize(S.s);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.e0, ev.e1);
    if (e != hipSuccess || hipGetLastError() != hipSuccess) return fnn::fail(FNN_EHIP, std::string("fnn_split_weights_f64: ") + hipGetErrorString(e));
    double kk[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t q = 0; q < kp.size(); q += 4)
        for (int a = 0; a < 4; a++) kk[a] = (kp[q + a] > kk[a] || kp[q + a] != kp[q + a]) ? kp[q + a] : kk[a];
    const double scale = kk[3] > 0.0 ? kk[3] : 1.0;
    const double viol = std::max({kk[0], kk[1] / scale, kk[2] / scale});
    const bool certified = viol <= 1e-9;  // (NaN compares false)
    // what goes back to the host: every weight, or only those above the threshold (the reference keeps x[k] > 1e-6, FastNN.java:455:
    // 77 000 of 5.4e8 weights at 32768 taxa - the dense array is 4.3 GB over the bus and a host pass over it)
    const int64_t Nw = (int64_t)n * (n - 1) / 2;
    int64_t npos = 0;
    {
        unsigned long long* dcount = S.alloc<unsigned long long>(1);
        const int64_t pcap = weights_out ? 0 : cap_out;
        int64_t* didx = S.alloc<int64_t>((size_t)std::max<int64_t>(pcap, 1));
        double* dw = S.alloc<double>((size_t)std::max<int64_t>(pcap, 1));
        if (!S.ok) return fnn::fail(FNN_ENOMEM, "fnn_split_weights_f64: device allocation failed");
        (void)hipMemsetAsync(dcount, 0, sizeof(unsigned long long), S.s);
        hipLaunchKernelGGL(k_pick_positive, dim3((unsigned)((Nw + T - 1) / T)), dim3(T), 0, S.s, S.live, Nw, weights_out ? 0.000001 : thr, didx, dw, dcount,
                           (unsigned long long)pcap);
        unsigned long long c = 0;
        if (!SWOK(hipMemcpyAsync(&c, dcount, sizeof(c), hipMemcpyDeviceToHost, S.s)) || !SWOK(hipStreamSynchronize(S.s)))
            return fnn::fail(FNN_EHIP, "fnn_split_weights_f64: download failed");
        npos = (int64_t)c;
        if (weights_out) {
            if (!SWOK(hipMemcpy(weights_out, S.live, sizeof(double) * (size_t)Nw, hipMemcpyDeviceToHost)))
                return fnn::fail(FNN_EHIP, "fnn_split_weights_f64: download failed");
        } else {
            *count_out = npos;
            const int64_t take = std::min(npos, cap_out);
            std::vector<int64_t> hi((size_t)take);
            std::vector<double> hw((size_t)take);
            if (take > 0 && (!SWOK(hipMemcpy(hi.data(), didx, sizeof(int64_t) * (size_t)take, hipMemcpyDeviceToHost)) ||
                             !SWOK(hipMemcpy(hw.data(), dw, sizeof(double) * (size_t)take, hipMemcpyDeviceToHost))))
                return fnn::fail(FNN_EHIP, "fnn_split_weights_f64: download failed");
            std::vector<int64_t> perm((size_t)take);
            for (int64_t q = 0; q < take; q++) perm[(size_t)q] = q;
            std::sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return hi[(size_t)a] < hi[(size_t)b]; });  // the reference's list order
            for (int64_t q = 0; q < take; q++) { idx_out[q] = hi[(size_t)perm[(size_t)q]]; w_out[q] = hw[(size_t)perm[(size_t)q]]; }
        }
    }
    const Outcome outcome{route, npos, certified, viol, ms * 1e-3};
    fill_stats(stats, S, &outcome);
    if (route == FNN_SW_ROUTE_FROM_BELOW && !certified) {
        char buf[320];
        std::snprintf(buf, sizeof(buf), "fnn_split_weights_f64: the weights fail the Kuhn-Tucker check: violation %.3g of max|A^T d| (min x %.3g, gradient on positive weights %.3g, "
                      "on zero weights %.3g; candidates' final threshold %.3g, %lld splits set aside): not the certified optimum",
                      viol, -kk[0], kk[1] / scale, kk[2] / scale, S.final_tol_rel, (long long)S.n_set_aside);
        std::fprintf(stderr, "%s\n", buf);
        return fnn::fail(FNN_EINEXACT, buf);
    }
    return FNN_OK;
}

extern "C" int32_t fnn_split_weights_f64(const double* D, int32_t n, int64_t ldD, const int32_t* ordering, int32_t device,
                                         double* weights_out, fnn_sw_stats* stats) {
    if (!weights_out) return fnn::fail(FNN_EINVAL, "fnn_split_weights_f64: bad arguments");
    return split_weights_impl(D, n, ldD, ordering, device, weights_out, 0.0, nullptr, nullptr, 0, nullptr, stats);
}
extern "C" int32_t fnn_split_weights_release_cache(void) {
    fnnsw::pool().flush();
    return FNN_OK;
}
extern "C" int32_t fnn_split_weights_sparse_f64(const double* D, int32_t n, int64_t ldD, const int32_t* ordering, int32_t device, double threshold,
                                                int64_t* index_out, double* weight_out, int64_t capacity, int64_t* count_out, fnn_sw_stats* stats) {
    return split_weights_impl(D, n, ldD, ordering, device, nullptr, threshold, index_out, weight_out, capacity, count_out, stats);
}
