// qm_traveltimes.hpp -- travel-time tables on the device (host side: qm_traveltimes.hip; the rules on arrays:
// tests/traveltimes_ref.py).  Three kernels, all float64 with contraction off, IEEE divide and square root:
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
// The two per-node kernels run one launch over all rows: kTtGridBlocks x kTtGridThreads threads stride over a row's
// nodes, row after row (32-bit index arithmetic; no shape depends on the launch grid).
#pragma once
#include "qm_block.hpp"

namespace qm {

constexpr int kTtLdsNodes = 20000;              // 8 bytes per node + the reduction's slots <= 160 KB
constexpr int kTtSectionThreads = 512;
constexpr int kTtGridBlocks = 2048, kTtGridThreads = 256;
constexpr unsigned long long kTtNone = ~0ull;

enum TtStage : int { kTtHomogeneous = 0, kTtSections, kTtSweep, kTtStages };
inline constexpr const char *const kTtStageNames[kTtStages] = {"homogeneous", "sections", "sweep"};

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

#ifdef QM_TU_TRAVELTIMES
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
