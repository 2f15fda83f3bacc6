// qm_traveltimes.hpp -- travel-time tables on the device (host side: qm_traveltimes.hip; the rules on arrays:
// tests/traveltimes_ref.py, tests/traveltimes3d_ref.py).  All float64 with contraction off, IEEE divide and square root:
//   tt_homogeneous_kernel   per (row, node): sqrt(dx*dx + dy*dy + dz*dz) / v (create_lut.py:262-265).  A store stream
//   tt_sections_kernel      |grad T| = s(z) on a (distance, depth) section, source in column 0: the multiplicatively
//                           factored first-order upwind scheme, T = T0 tau with T0 = s0 rho the homogeneous solution
//                           for the slowness at the source.  Gauss-Seidel sweeps in four orderings until a round of
//                           four accepts nothing.  ONE WORKGROUP PER SECTION, every anti-diagonal of a sweep in
//                           parallel, one barrier per diagonal: a node of diagonal d reads diagonal d - 1 as this
//                           sweep left it and d + 1 as it found it, which is what the serial i-outer / k-inner loop
//                           reads -- the values are that loop's, bit for bit.  tau lives in LDS up to kTtLdsNodes
//                           nodes, above that in the engine's scratch (L2-resident: a section is a few MB): the same
//                           arithmetic, the same bits.  No workgroup waits on another, no atomics.
//                           A few dozen sections on 256 CUs: this is a latency problem -- (nr + nz - 1) x 4 dependent
//                           steps per round, each a barrier and a chain of divides and square roots -- not a
//                           throughput one, and the launch is not shaped for occupancy.
//   tt_sweep_kernel         per (row, node): distance and depth of the node from the row's station, then the
//                           reference's _bilinear_interpolate (create_lut.py:746-762) on the row's section, literally:
//                           floor of the offsets from the origin for the cell, np.remainder of the COORDINATES for the
//                           fractions.  A node whose cell leaves the section is reported (the smallest such node per
//                           row, by an atomic minimum nobody waits on) and gets NaN.
//   tt_eikonal_*_kernel     |grad T| = s(x, y, z) on the 3-D node grid itself, one solve per row, the source anywhere
//                           inside the grid: the section kernel's scheme with one axis more (tt_update3 below has the
//                           order of its operations).  Gauss-Seidel sweeps in eight orderings.  ONE LAUNCH PER PLANE
//                           i' + j' + k' = d of a sweep (indices after the ordering's reflection), all rows in it: a
//                           node's six neighbours lie in the planes d - 1 and d + 1, never in its own, so a plane at
//                           once reads what the serial x-outer / z-inner loop reads and the values are that loop's, bit
//                           for bit.  Stream order is the only dependency between planes -- a kernel boundary is what
//                           makes one plane's stores visible to the next on every XCD: no workgroup waits on another,
//                           no barriers, no atomics; a row's "accepted something" flag is a plain store of 1.  tau
//                           lives in place in the output rows, T0 and its gradient are recomputed per update from the
//                           coordinates.  8 (nx + ny + nz - 2) launches per round, one flag read-back per round.  The
//                           launch covers the bounding rectangle of the plane in (i', j'), a thread per (i', j') and
//                           so one node at most per thread: nothing depends on the launch grid.  A row the previous
//                           round settled leaves at once (its further rounds change nothing).  Planes near the
//                           corners are nearly empty and a plane's nodes lie nz - 1 doubles apart: the launch train
//                           and the uncoalesced access are accepted here (no plane-major layout, no fused corner
//                           planes).  Measured: at 201 x 201 x 101 x 60 rows the rows' arithmetic
//                           bounds a call, at 71 x 64 x 57 x 24 rows the launch train does (8 us a launch).
// The per-node kernels run one launch over all rows: kTtGridBlocks x kTtGridThreads threads stride over a row's
// nodes, row after row (32-bit index arithmetic; no shape depends on the launch grid).
#pragma once
#include "qm_block.hpp"

namespace qm {

constexpr int kTtLdsNodes = 20000;              // 8 bytes per node + the reduction's slots <= 160 KB
constexpr int kTtSectionThreads = 512;
constexpr int kTtGridBlocks = 2048, kTtGridThreads = 256;
constexpr int kTtPlaneThreads = 256;            // a workgroup of the plane launch: one (i', j') of the plane's rectangle per thread
constexpr int kTtPlaneMaxRows = 65535;          // rows ride in the launch grid's y
constexpr unsigned long long kTtNone = ~0ull;

enum TtStage : int { kTtHomogeneous = 0, kTtSections, kTtSweep, kTtEikonal3d, kTtStages };
inline constexpr const char *const kTtStageNames[kTtStages] = {"homogeneous", "sections", "sweep", "eikonal3d"};

struct TtGrid {
    double ll[3], sp[3];
    int n[3];
    long long nodes, total;                     // nodes of a grid (< 2^31); rows x nodes
    int rows;
};
struct TtSectionArgs {
    const double *slow;                         // [n_sections][nz]
    const double *src;                          // [n_sections][2]: source depth below row 0, slowness at the source
    double *T;                                  // [n_sections][nr][nz]
    double *scratch;                            // the same shape: tau above the LDS limit
    int32_t *rounds, *status;
    int nr, nz, max_iters;
    double h, tol;
};
struct TtSweepArgs {
    TtGrid g;
    const double *rows;                         // [n_rows][4]: station x, y; section origin x0, z0
    const int32_t *row_sec;
    const double *sections;                     // [n_sections][nr][nz]
    int nr, nz;
    double h;
    double *out;
    unsigned long long *bad;                    // [n_rows]: the smallest node outside its section, kTtNone: none
};
struct TtEikonalArgs {
    TtGrid g;
    const double *rows;                         // [n_rows][4]: source x, y, z; slowness at the source
    const int32_t *row_model;                   // [n_rows]
    const int32_t *cell;                        // [n_rows][3]: the cell that holds the source; its eight nodes are frozen
    const double *slow;                         // [n_models][nodes]
    double *tau;                                // [n_rows][nodes]: the output rows; tau until the last pass forms T
    const int32_t *live;                        // [n_rows]: the row accepted something in the previous round
    int32_t *flag;                              // [n_rows]: ... in this one
    double tol;
};
struct TtPlane {                                // one plane of one sweep
    int rev[3];                                 // the ordering runs this axis backwards
    int d;                                      // i' + j' + k'
    int lo0, n0, lo1, n1;                       // the plane's bounding rectangle in (i', j')
};
using TtReduce = BlockReduce<1, kTtSectionThreads / 64>;
inline size_t tt_lds_bytes(long long nodes) { return (size_t)nodes * sizeof(double); }

// np.remainder for doubles: fmod, + b where the signs differ, a zero keeps b's sign
__device__ __forceinline__ double tt_remainder(double a, double b) {
#pragma clang fp contract(off)
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

// node `node` of the grid: its three coordinates, ll + index * spacing (Grid3D.grid_xyz)
__device__ __forceinline__ void tt_node_xyz(const TtGrid &g, unsigned node, double &x, double &y, double &z) {
#pragma clang fp contract(off)
    const unsigned t = node / (unsigned)g.n[2];
    const int iz = (int)(node - t * (unsigned)g.n[2]);
    const int ix = (int)(t / (unsigned)g.n[1]);
    const int iy = (int)(t - (unsigned)ix * (unsigned)g.n[1]);
    x = g.ll[0] + (double)ix * g.sp[0];
    y = g.ll[1] + (double)iy * g.sp[1];
    z = g.ll[2] + (double)iz * g.sp[2];
}

// one neighbour along one axis: alpha, beta, whether it is available, and its one-sided candidate into `best`
__device__ __forceinline__ void tt_side(double sg, double ta, double t0, double t0d, double h, double sk, double &a,
                                        double &b, bool &av, double &best) {
#pragma clang fp contract(off)
    av = ta < __builtin_inf();
    a = t0 * sg / h + t0d;
    b = t0 * sg * ta / h;
    const double t = (b + sg * sk) / a;
    if (av && sg * a > 0.0 && t > 0.0 && t < best) best = t;
}
// the two-sided candidate of a horizontal and a vertical neighbour: the larger root, kept under the two sign tests
__device__ __forceinline__ void tt_pair(double sx, double ax, double bx, bool avx, double sz, double az, double bz,
                                        bool avz, double sk, double &best) {
#pragma clang fp contract(off)
    const double qa = ax * ax + az * az;
    const double qb = ax * bx + az * bz;
    const double qc = bx * bx + bz * bz - sk * sk;
    const double disc = qb * qb - qa * qc;
    const double t = (qb + sqrt(disc)) / qa;
    if (avx && avz && disc >= 0.0 && sx * (ax * t - bx) >= 0.0 && sz * (az * t - bz) >= 0.0 && t < best) best = t;
}

// the three-sided candidate: tt_pair with one axis more, every sum taken left to right
__device__ __forceinline__ void tt_triple(double sx, double ax, double bx, bool avx, double sy, double ay, double by,
                                          bool avy, double sz, double az, double bz, bool avz, double sk, double &best) {
#pragma clang fp contract(off)
    const double qa = ax * ax + ay * ay + az * az;
    const double qb = ax * bx + ay * by + az * bz;
    const double qc = bx * bx + by * by + bz * bz - sk * sk;
    const double disc = qb * qb - qa * qc;
    const double t = (qb + sqrt(disc)) / qa;
    if (avx && avy && avz && disc >= 0.0 && sx * (ax * t - bx) >= 0.0 && sy * (ay * t - by) >= 0.0 &&
        sz * (az * t - bz) >= 0.0 && t < best)
        best = t;
}

// node (i, j, k) seen from a row's source r = (x, y, z, s0): T0 = s0 rho and its three derivatives s0 d / rho, with
// d = (ll + index * spacing) - source per axis and rho = sqrt(dx dx + dy dy + dz dz), the sum left to right
__device__ __forceinline__ double tt_t0(const TtGrid &g, const double *r, int i, int j, int k, double (&t0d)[3]) {
#pragma clang fp contract(off)
    const double dx = (g.ll[0] + (double)i * g.sp[0]) - r[0];
    const double dy = (g.ll[1] + (double)j * g.sp[1]) - r[1];
    const double dz = (g.ll[2] + (double)k * g.sp[2]) - r[2];
    const double rho = sqrt(dx * dx + dy * dy + dz * dz);
    t0d[0] = r[3] * dx / rho;
    t0d[1] = r[3] * dy / rho;
    t0d[2] = r[3] * dz / rho;
    return r[3] * rho;
}

// The 3-D node update, in this order: the 6 one-sided candidates -- x from index - 1 (sg = +1), x from index + 1
// (sg = -1), then y, then z --, the 12 two-sided ones -- axes (x, y), (x, z), (y, z), per pair the sides (+,+) (+,-)
// (-,+) (-,-) --, the 8 three-sided ones, sides of x outermost.  nb[d][side]: tau of the neighbour, +inf where there is
// none.  Returns the smallest candidate kept, +inf: none.
__device__ __forceinline__ double tt_update3(const double (&nb)[3][2], double t0, const double (&t0d)[3],
                                             const double (&h)[3], double sk) {
#pragma clang fp contract(off)
    double best = __builtin_inf(), a[3][2], b[3][2];
    bool av[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int p = 0; p < 2; ++p) tt_side(p ? -1.0 : 1.0, nb[d][p], t0, t0d[d], h[d], sk, a[d][p], b[d][p], av[d][p], best);
#pragma unroll
    for (int pr = 0; pr < 3; ++pr) {
        const int d = pr == 2 ? 1 : 0, e = pr == 0 ? 1 : 2;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q)
                tt_pair(p ? -1.0 : 1.0, a[d][p], b[d][p], av[d][p], q ? -1.0 : 1.0, a[e][q], b[e][q], av[e][q], sk, best);
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 2; ++r)
                tt_triple(p ? -1.0 : 1.0, a[0][p], b[0][p], av[0][p], q ? -1.0 : 1.0, a[1][q], b[1][q], av[1][q],
                          r ? -1.0 : 1.0, a[2][r], b[2][r], av[2][r], sk, best);
    return best;
}

// is node (i, j, k) one of the eight nodes of cell c?
__device__ __forceinline__ bool tt_in_box(const int32_t *c, int i, int j, int k) {
    return (i == c[0] || i == c[0] + 1) && (j == c[1] || j == c[1] + 1) && (k == c[2] || k == c[2] + 1);
}

#ifdef QM_TU_TRAVELTIMES
// the smallest element of `slow` that is not finite and positive (kTtNone stays: there is none); nobody waits on the
// atomic minimum
__global__ __launch_bounds__(kTtGridThreads) void tt_slowness_check_kernel(const double *slow, unsigned long long n,
                                                                           unsigned long long *bad) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double v = slow[i];
        if (!(v > 0.0 && v < __builtin_inf())) atomicMin(bad, i);
    }
}

// tau before the first sweep: +inf, the source's box frozen at (s0 + s) / (2 s0), a node at the source itself at 1
__global__ __launch_bounds__(kTtGridThreads) void tt_eikonal_init_kernel(TtEikonalArgs a) {
#pragma clang fp contract(off)
    const unsigned stride = gridDim.x * blockDim.x, nodes = (unsigned)a.g.nodes;
    for (int row = 0; row < a.g.rows; ++row) {
        const double *r = a.rows + 4 * row;
        const int32_t *c = a.cell + 3 * row;
        const double *slow = a.slow + (size_t)a.row_model[row] * nodes;
        double *tau = a.tau + (size_t)row * nodes;
        for (unsigned node = blockIdx.x * blockDim.x + threadIdx.x; node < nodes; node += stride) {
            const unsigned t = node / (unsigned)a.g.n[2];
            const int k = (int)(node - t * (unsigned)a.g.n[2]), i = (int)(t / (unsigned)a.g.n[1]);
            const int j = (int)(t - (unsigned)i * (unsigned)a.g.n[1]);
            double v = __builtin_inf();
            if (tt_in_box(c, i, j, k)) {
                double t0d[3];
                v = tt_t0(a.g, r, i, j, k, t0d) == 0.0 ? 1.0 : (r[3] + slow[node]) / (2.0 * r[3]);
            }
            tau[node] = v;
        }
    }
}

// one plane of one sweep, all rows: grid (the plane's rectangle / kTtPlaneThreads, n_rows)
__global__ __launch_bounds__(kTtPlaneThreads) void tt_eikonal_plane_kernel(TtEikonalArgs a, TtPlane p) {
#pragma clang fp contract(off)
    const int row = blockIdx.y;
    if (!a.live[row]) return;                       // settled by the previous round: this one would change nothing
    const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (unsigned)p.n0 * (unsigned)p.n1) return;
    const int nx = a.g.n[0], ny = a.g.n[1], nz = a.g.n[2];
    const int ip = p.lo0 + (int)(c / (unsigned)p.n1), jp = p.lo1 + (int)(c % (unsigned)p.n1), kp = p.d - ip - jp;
    if (ip >= nx || jp >= ny || kp < 0 || kp >= nz) return;
    const int i = p.rev[0] ? nx - 1 - ip : ip, j = p.rev[1] ? ny - 1 - jp : jp, k = p.rev[2] ? nz - 1 - kp : kp;
    if (tt_in_box(a.cell + 3 * row, i, j, k)) return;
    const unsigned nodes = (unsigned)a.g.nodes, node = ((unsigned)i * (unsigned)ny + (unsigned)j) * (unsigned)nz + (unsigned)k;
    double *at = a.tau + (size_t)row * nodes + node;
    const double inf = __builtin_inf();
    const ptrdiff_t sx = (ptrdiff_t)ny * nz, sy = nz;
    const double nb[3][2] = {{i > 0 ? at[-sx] : inf, i < nx - 1 ? at[sx] : inf},
                             {j > 0 ? at[-sy] : inf, j < ny - 1 ? at[sy] : inf},
                             {k > 0 ? at[-1] : inf, k < nz - 1 ? at[1] : inf}};
    const double h[3] = {a.g.sp[0], a.g.sp[1], a.g.sp[2]};
    double t0d[3];
    const double t0 = tt_t0(a.g, a.rows + 4 * row, i, j, k, t0d);
    const double sk = a.slow[(size_t)a.row_model[row] * nodes + node];
    const double old = *at;
    const double best = tt_update3(nb, t0, t0d, h, sk);
    // taken only where it is below the old value by more than tol * old
    if (best < old && (old == inf || old - best > a.tol * old)) {
        *at = best;
        a.flag[row] = 1;
    }
}

// the last pass: T = T0 tau in place, 0 at the source
__global__ __launch_bounds__(kTtGridThreads) void tt_eikonal_finish_kernel(TtEikonalArgs a) {
#pragma clang fp contract(off)
    const unsigned stride = gridDim.x * blockDim.x, nodes = (unsigned)a.g.nodes;
    for (int row = 0; row < a.g.rows; ++row) {
        const double *r = a.rows + 4 * row;
        double *tau = a.tau + (size_t)row * nodes;
        for (unsigned node = blockIdx.x * blockDim.x + threadIdx.x; node < nodes; node += stride) {
            const unsigned t = node / (unsigned)a.g.n[2];
            const int k = (int)(node - t * (unsigned)a.g.n[2]), i = (int)(t / (unsigned)a.g.n[1]);
            const int j = (int)(t - (unsigned)i * (unsigned)a.g.n[1]);
            double t0d[3];
            const double t0 = tt_t0(a.g, r, i, j, k, t0d);
            tau[node] = t0 == 0.0 ? 0.0 : t0 * tau[node];
        }
    }
}

__global__ __launch_bounds__(kTtGridThreads) void tt_homogeneous_kernel(TtGrid g, const double *rows, double *out) {
#pragma clang fp contract(off)
    // (row by row, the launch grid striding over a row's nodes: no 64-bit division per node)
    const unsigned stride = gridDim.x * blockDim.x, nodes = (unsigned)g.nodes;
    for (int row = 0; row < g.rows; ++row) {
        const double *r = rows + 4 * row;
        double *o = out + (size_t)row * nodes;
        for (unsigned node = blockIdx.x * blockDim.x + threadIdx.x; node < nodes; node += stride) {
            double x, y, z;
            tt_node_xyz(g, node, x, y, z);
            const double dx = x - r[0], dy = y - r[1], dz = z - r[2];
            const double dist = sqrt(dx * dx + dy * dy + dz * dz);
            o[node] = dist / r[3];
        }
    }
}

__global__ __launch_bounds__(kTtGridThreads) void tt_sweep_kernel(TtSweepArgs a) {
#pragma clang fp contract(off)
    const unsigned stride = gridDim.x * blockDim.x, nodes = (unsigned)a.g.nodes;
    for (int row = 0; row < a.g.rows; ++row) {
        const double *r = a.rows + 4 * row;
        const double *sec = a.sections + (size_t)a.row_sec[row] * a.nr * a.nz;
        double *o = a.out + (size_t)row * nodes;
        for (unsigned node = blockIdx.x * blockDim.x + threadIdx.x; node < nodes; node += stride) {
            double x, y, z;
            tt_node_xyz(a.g, node, x, y, z);
            const double dx = x - r[0], dy = y - r[1];
            const double d = sqrt(dx * dx + dy * dy);
            const double fi = floor((d - r[2]) / a.h), fk = floor((z - r[3]) / a.h);
            if (!(fi >= 0.0 && fi <= (double)(a.nr - 2) && fk >= 0.0 && fk <= (double)(a.nz - 2))) {
                atomicMin(&a.bad[row], (unsigned long long)node);
                o[node] = __builtin_nan("");
                continue;
            }
            const int i = (int)fi, k = (int)fk;
            const double xd = tt_remainder(d, a.h) / a.h, zd = tt_remainder(z, a.h) / a.h;
            const double *c = sec + (size_t)i * a.nz + k;
            const double c00 = c[0], c01 = c[1], c10 = c[a.nz], c11 = c[a.nz + 1];
            const double c0 = c00 * (1.0 - xd) + c10 * xd;
            const double c1 = c01 * (1.0 - xd) + c11 * xd;
            o[node] = c0 * (1.0 - zd) + c1 * zd;
        }
    }
}

template <bool kLds>
__global__ __launch_bounds__(kTtSectionThreads) void tt_sections_kernel(TtSectionArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double tt_tau_lds[];
    __shared__ unsigned long long red_slots[TtReduce::kWords];
    const int sec = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const int nr = a.nr, nz = a.nz;
    const int n = nr * nz;
    double *tau = kLds ? tt_tau_lds : a.scratch + (size_t)sec * n;
    const double *slow = a.slow + (size_t)sec * nz;
    const double zsrc = a.src[2 * sec], s0 = a.src[2 * sec + 1];
    const double h = a.h, tol = a.tol, inf = __builtin_inf();
    const int k0 = (int)floor(zsrc / h);            // the source box: columns 0, 1 of rows k0, k0 + 1 (checked: inside)

    for (int idx = tid; idx < n; idx += threads) {
        const int i = idx / nz, k = idx - i * nz;
        double v = inf;
        if (i <= 1 && (k == k0 || k == k0 + 1)) {
            const double x = (double)i * h, z = (double)k * h - zsrc;
            v = (x * x + z * z == 0.0) ? 1.0 : (s0 + slow[k]) / (2.0 * s0);
        }
        tau[idx] = v;
    }
    __syncthreads();

    TtReduce red{red_slots, threads >> 6, 0};
    int rounds = 0;
    bool settled = false;
    while (rounds < a.max_iters) {
        long long any[1] = {0};
        for (int o = 0; o < 4; ++o) {               // (+,+) (-,+) (-,-) (+,-) of (i, k)
            const bool ifwd = o == 0 || o == 3, kfwd = o < 2;
            for (int d = 0; d < nr + nz - 1; ++d) {
                const int lo = d - nz + 1 > 0 ? d - nz + 1 : 0, hi = d < nr - 1 ? d : nr - 1;
                for (int ip = lo + tid; ip <= hi; ip += threads) {
                    const int i = ifwd ? ip : nr - 1 - ip, k = kfwd ? d - ip : nz - 1 - (d - ip);
                    if (i <= 1 && (k == k0 || k == k0 + 1)) continue;
                    const double x = (double)i * h, z = (double)k * h - zsrc;
                    const double rho = sqrt(x * x + z * z);
                    const double t0 = s0 * rho, t0x = s0 * x / rho, t0z = s0 * z / rho;
                    const double sk = slow[k];
                    double *at = tau + (size_t)i * nz + k;
                    const double old = *at;
                    double best = inf, ax[2], bx[2], az[2], bz[2];
                    bool avx[2], avz[2];
                    tt_side(1.0, i > 0 ? at[-nz] : inf, t0, t0x, h, sk, ax[0], bx[0], avx[0], best);
                    tt_side(-1.0, i < nr - 1 ? at[nz] : inf, t0, t0x, h, sk, ax[1], bx[1], avx[1], best);
                    tt_side(1.0, k > 0 ? at[-1] : inf, t0, t0z, h, sk, az[0], bz[0], avz[0], best);
                    tt_side(-1.0, k < nz - 1 ? at[1] : inf, t0, t0z, h, sk, az[1], bz[1], avz[1], best);
#pragma unroll
                    for (int p = 0; p < 2; ++p)
#pragma unroll
                        for (int q = 0; q < 2; ++q)
                            tt_pair(p ? -1.0 : 1.0, ax[p], bx[p], avx[p], q ? -1.0 : 1.0, az[q], bz[q], avz[q], sk, best);
                    // taken only where it is below the old value by more than tol * old
                    if (best < old && (old == inf || old - best > tol * old)) {
                        *at = best;
                        any[0] = 1;
                    }
                }
                __syncthreads();
            }
        }
        red.run(any, BlockMax());
        ++rounds;
        if (!any[0]) {
            settled = true;
            break;
        }
    }

    double *T = a.T + (size_t)sec * n;
    for (int idx = tid; idx < n; idx += threads) {
        const int i = idx / nz, k = idx - i * nz;
        const double x = (double)i * h, z = (double)k * h - zsrc;
        const double t0 = s0 * sqrt(x * x + z * z);
        T[idx] = t0 == 0.0 ? 0.0 : t0 * tau[idx];
    }
    if (tid == 0) {
        a.rounds[sec] = rounds;
        a.status[sec] = settled ? 0 : 1;
    }
}
#endif  // QM_TU_TRAVELTIMES

}  // namespace qm
