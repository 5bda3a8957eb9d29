// The TLS fit of Schomaker & Trueblood (Acta Cryst. B24 (1968) 63) on predicted ADPs: per molecule of a batch the
// translation tensor T, the libration tensor L and the screw tensor S of the rigid body that explains the molecule's ADPs
// best, U(r) = T + A L A^T + A S + S^T A^T with A(r) = [[0, z, -y], [-z, 0, x], [y, -x, 0]], and what is left per atom.
// The reference has no counterpart: its only statements about a prediction need the truth (main.py:47-49).  The rule is
// stated in cartnet_amd/bonds.py and restated there in numpy (tls_fit_host); the molecules are cartnet_molecules'.
//
//   cn_tls_fit_kernel   grid (B, TLS_SLOTS), 512 threads.  Workgroup (g, s) first gives the rows of crystal g that belong to
//                       unfitted molecules (status != 0 or fewer than TLS_MIN_ATOMS atoms: a row knows both) their neutral
//                       values, the rows strided over the slots.  Then it walks the roots of the crystal in atom order
//                       (label[i] == i; every wave takes the same ballots, so all threads agree without a barrier) and
//                       fits molecule number k when k % TLS_SLOTS == s:
//     geometry   c and rho by two ballot-and-shuffle scans of the crystal's atoms, members folded in atom order; every wave
//                computes the same bits, so the whole workgroup branches alike.
//     normal     the members of 64 atoms are listed in LDS by wave 0; TLS_STAGE of them at a time have their J_i (6 x 20)
//                and y_i staged in LDS, one thread per entry; then one thread per entry of N (400) adds J_i^T J_i, twenty
//                add J_i^T y_i and one adds |y_i|^2, atom after atom.
//     jacobi     N and V in LDS.  A sweep is the 19 rounds of the round-robin ordering; in a round each of the 20 indices
//                computes its pair's (c, s) from N as the round found it, then one thread per entry forms
//                (G^T N G)_ij from four entries and (V G)_ij from two, all rotations of the round together.  Before each
//                sweep every thread sums the same off-diagonal and diagonal squares: a uniform decision.  At most
//                TLS_MAX_SWEEPS sweeps; a molecule that uses them up gets rank -1 and NaN.
//     solve      p = V_kept diag(1 / lambda) V_kept^T b over the eigenvalues above TLS_RANK_EPS lambda_max, unscaled to T,
//                L, S about c; the principal values of T and L by the same routine at n = 3.
//     rows       one thread per member: u_tls = U(r_i), resid = |Sym U_i - u_tls|_F; the sum of resid^2 is folded by a
//                butterfly per wave and then over the waves in order.  A last scan replicates params, eig, rank and rfac
//                on every row of the molecule.
//   cn_tls_crystal_kernel   one wave per crystal (crystal_reduce.h) over its atoms: fitted molecules (rank != 0, at roots),
//                       those with rank < 20, those with a negative smallest principal value of T or L, and over the rows
//                       of fitted molecules the sum of resid^2 as stored, the sum of |Sym U|_F^2 and the largest resid.
//
// No atomics, no workgroup waits for another, fixed order: two runs give the same bytes.  64-bit offsets throughout.
// Nothing that is indexed dynamically lives in registers: N, V, J_i, b and p are in LDS (about 12 KB); no scratch.
#include "bond_graph.h"

namespace {

constexpr int TLS_THREADS = 512;
constexpr int TLS_WAVES = TLS_THREADS / WAVE;
constexpr int TLS_SLOTS = 8;                     // workgroups per crystal: molecule k belongs to slot k % TLS_SLOTS
constexpr int TLS_P = 20;                        // parameters: T (6), L (6), S (8)
constexpr int TLS_MIN_ATOMS = 5;
constexpr int TLS_MAX_SWEEPS = 30;
constexpr int TLS_STAGE = 4;                     // atoms whose J_i are staged at a time: 4 * 126 entries <= 512 threads
constexpr int TLS_ENTRIES = 6 * TLS_P + 6;       // of one staged atom: J_i and y_i
constexpr double TLS_RANK_EPS = 1e-10;
constexpr double TLS_JACOBI_TOL = 1e-15;
constexpr double TLS_SQRT2 = 1.4142135623730951;

static_assert(TLS_STAGE * TLS_ENTRIES <= TLS_THREADS && TLS_P * TLS_P + TLS_P + 1 <= TLS_THREADS, "one thread per entry");

struct TlsShared {
  double n[TLS_P * TLS_P];                       // the normal matrix; later T, then L, for their principal values
  double v[TLS_P * TLS_P];                       // the eigenvectors
  double j[TLS_STAGE][6][TLS_P];                 // the staged J_i
  double y[TLS_STAGE][6];                        // ... and y_i
  double b[TLS_P], p[TLS_P], coef[TLS_P];
  double cc[TLS_P], ss[TLS_P], row[TLS_P];       // a round's rotations per index; a sweep's off-diagonal row sums
  double mol[30];                                // T, L, S row-major (unscaled) and c
  double eig[6];
  double fold[TLS_WAVES];
  double sym2;
  int partner[TLS_P], turn[TLS_P];
  int members[WAVE];
  int count, rank;
};

// the pair (p, q) of observation / parameter o in the order 11 22 33 23 13 12
__device__ __forceinline__ int tls_p(int o) { return o < 3 ? o : (o == 3 ? 1 : 0); }
__device__ __forceinline__ int tls_q(int o) { return o < 3 ? o : (o == 5 ? 1 : 2); }
// the entry (m, n) of S's parameter k in the order 11 22 12 13 21 23 31 32
__device__ __forceinline__ int tls_sm(int k) { return k < 2 ? k : (k < 4 ? 0 : (k < 6 ? 1 : 2)); }
__device__ __forceinline__ int tls_sn(int k) {
  return k < 2 ? k : (k == 2 ? 1 : (k == 3 ? 2 : (k == 4 ? 0 : (k == 5 ? 2 : (k == 6 ? 0 : 1)))));
}

// A(r)[p][m] by selects: no table in registers
__device__ __forceinline__ double tls_a(int p, int m, double x, double y, double z) {
  const int k = p * 3 + m;
  return k == 1 ? z : (k == 2 ? -y : (k == 3 ? -z : (k == 5 ? x : (k == 6 ? y : (k == 7 ? -x : 0.0)))));
}

// J_i[o][a] for the (scaled) position (x, y, z): w_pq dU_pq / dparam_a
__device__ __forceinline__ double tls_design(int o, int a, double x, double y, double z) {
  const int p = tls_p(o), q = tls_q(o);
  const double w = o < 3 ? 1.0 : TLS_SQRT2;
  if (a < 6) return a == o ? w : 0.0;
  if (a < 12) {                                                      // (A E A^T)_pq, E symmetric
    const int m = tls_p(a - 6), n = tls_q(a - 6);
    const double pm = tls_a(p, m, x, y, z), qn = tls_a(q, n, x, y, z);
    if (m == n) return w * (pm * qn);
    return w * (pm * qn + tls_a(p, n, x, y, z) * tls_a(q, m, x, y, z));
  }
  const int k = a - 12, m = tls_sm(k), n = tls_sn(k);                 // (A E + (A E)^T)_pq; a diagonal E carries -E_33
  double v = (n == q ? tls_a(p, m, x, y, z) : 0.0) + (n == p ? tls_a(q, m, x, y, z) : 0.0);
  if (k < 2) v -= (q == 2 ? tls_a(p, 2, x, y, z) : 0.0) + (p == 2 ? tls_a(q, 2, x, y, z) : 0.0);
  return w * v;
}

struct TlsOut {
  float* __restrict__ u_tls;
  float* __restrict__ resid;
  float* __restrict__ params;
  float* __restrict__ eig;
  int32_t* __restrict__ rank;
  float* __restrict__ rfac;
};

// a row without a fit: NaN tensors; (0, 0, 0) for an unfitted molecule, (NaN, -1, NaN) for one whose sweeps ran out
__device__ __forceinline__ void tls_blank(const TlsOut& out, int64_t m, float resid, int32_t rank) {
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int q = 0; q < 9; ++q) out.u_tls[m * 9 + q] = nan;
#pragma unroll
  for (int q = 0; q < 24; ++q) out.params[m * 24 + q] = nan;
#pragma unroll
  for (int q = 0; q < 6; ++q) out.eig[m * 6 + q] = nan;
  out.resid[m] = resid;
  out.rank[m] = rank;
  out.rfac[m] = resid;
}

// Cyclic Jacobi on sh.n (n x n, row stride TLS_P) with the eigenvectors in sh.v; called by the whole workgroup.  Returns
// the sweeps taken, or -1 when TLS_MAX_SWEEPS did not do; the same value in every thread.
__device__ int tls_jacobi(TlsShared& sh, int n, int tid) {
  const int even = n + (n & 1), rounds = even - 1;
  const int i = tid / TLS_P, j = tid - i * TLS_P;
  const bool entry = tid < TLS_P * TLS_P && i < n && j < n;
  if (entry) sh.v[tid] = i == j ? 1.0 : 0.0;
  __syncthreads();
#pragma unroll 1
  for (int sweep = 0;; ++sweep) {
    if (tid < n) {
      double s = 0.0;
      for (int c = 0; c < n; ++c) {
        const double a = sh.n[tid * TLS_P + c];
        s += c == tid ? 0.0 : a * a;
      }
      sh.row[tid] = s;
    }
    __syncthreads();
    double off = 0.0, diag = 0.0;
    for (int t = 0; t < n; ++t) {                                     // every thread the same sums: a uniform decision
      const double d = sh.n[t * TLS_P + t];
      off += sh.row[t];
      diag += d * d;
    }
    if (off <= TLS_JACOBI_TOL * TLS_JACOBI_TOL * diag) return sweep;
    if (sweep == TLS_MAX_SWEEPS) return -1;
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
      if (tid < n) {
        int other = tid == r ? rounds : (tid == rounds ? r : (2 * r - tid + rounds) % rounds);
        if (other >= n) other = tid;                                 // the bye of an odd n
        const int p = tid < other ? tid : other, q = tid < other ? other : tid;
        const double app = sh.n[p * TLS_P + p], aqq = sh.n[q * TLS_P + q], apq = sh.n[p * TLS_P + q];
        const bool turn = p != q && apq != 0.0;
        double c = 1.0, s = 0.0;
        if (turn) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
        }
        sh.cc[tid] = c;
        sh.ss[tid] = tid == p ? -s : s;                              // column j of N G: c N_j + s_j N_j'
        sh.partner[tid] = other;
        sh.turn[tid] = turn ? 1 : 0;
      }
      __syncthreads();
      double nn = 0.0, vv = 0.0;
      if (entry) {
        const int io = sh.partner[i], jo = sh.partner[j];
        const double ci = sh.cc[i], si = sh.ss[i], cj = sh.cc[j], sj = sh.ss[j];
        const double b0 = sh.n[i * TLS_P + j] * cj + sh.n[i * TLS_P + jo] * sj;
        const double b1 = sh.n[io * TLS_P + j] * cj + sh.n[io * TLS_P + jo] * sj;
        nn = b0 * ci + b1 * si;
        if (jo == i && sh.turn[i]) nn = 0.0;                         // the entry the rotation annihilates
        vv = sh.v[i * TLS_P + j] * cj + sh.v[i * TLS_P + jo] * sj;
      }
      __syncthreads();
      if (entry) {
        sh.n[tid] = nn;
        sh.v[tid] = vv;
      }
      __syncthreads();
    }
  }
}

// the principal values of the symmetric 3x3 at sh.mol[at] into sh.eig[to ... to + 2], ascending; NaN if the sweeps ran out
__device__ void tls_principal(TlsShared& sh, int at, int to, int tid) {
  if (tid < 9) sh.n[(tid / 3) * TLS_P + tid % 3] = sh.mol[at + tid];
  __syncthreads();
  const int sweeps = tls_jacobi(sh, 3, tid);
  if (tid == 0) {
    double a = sh.n[0], b = sh.n[TLS_P + 1], c = sh.n[2 * TLS_P + 2], t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
    const double nan = __builtin_nan("");
    sh.eig[to] = sweeps < 0 ? nan : a;
    sh.eig[to + 1] = sweeps < 0 ? nan : b;
    sh.eig[to + 2] = sweeps < 0 ? nan : c;
  }
  __syncthreads();
}

__global__ __launch_bounds__(TLS_THREADS) void cn_tls_fit_kernel(
    const float* __restrict__ u, const int64_t* __restrict__ label, const double* __restrict__ x,
    const int64_t* __restrict__ atom_row, const int64_t* __restrict__ ptr, const int32_t* __restrict__ mol_status,
    const int32_t* __restrict__ mol_size, int64_t N, int64_t M, TlsOut out) {
  __shared__ TlsShared sh;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int slot = blockIdx.y;
  int64_t a0, a1;
  cr_rows(ptr, blockIdx.x, N, a0, a1);

  // ---- the rows of unfitted molecules, strided over the slots
  for (int64_t i = a0 + (int64_t)slot * TLS_THREADS + tid; i < a1; i += (int64_t)TLS_SLOTS * TLS_THREADS) {
    const int64_t m = bg_row(atom_row, i, M);
    if (m >= 0 && !(mol_status[m] == 0 && mol_size[m] >= TLS_MIN_ATOMS)) tls_blank(out, m, 0.0f, 0);
  }

  // ---- the roots in atom order; every wave takes the same ballots
  int number = 0;
#pragma unroll 1
  for (int64_t walk = a0; walk < a1; walk += WAVE) {
    const int64_t cand = walk + lane;
    unsigned long long roots = __ballot(cand < a1 && label[cand] == cand && bg_row(atom_row, cand, M) >= 0);
#pragma unroll 1
    while (roots) {
      const int64_t root = walk + __builtin_ctzll(roots);
      roots &= roots - 1;
      const bool mine = number % TLS_SLOTS == slot;
      number += 1;
      if (!mine) continue;
      const int64_t mr = bg_row(atom_row, root, M);
      if (!(mol_status[mr] == 0 && mol_size[mr] >= TLS_MIN_ATOMS)) continue;

      // ---- geometry: c, then rho, the members folded in atom order
      double c[3] = {0.0, 0.0, 0.0};
      int atoms = 0;
#pragma unroll 1
      for (int64_t base = a0; base < a1; base += WAVE) {
        const int64_t i = base + lane;
        const bool member = i < a1 && label[i] == root && bg_row(atom_row, i, M) >= 0;
        double xi[3] = {0.0, 0.0, 0.0};
        if (member) {
#pragma unroll
          for (int q = 0; q < 3; ++q) xi[q] = x[i * 3 + q];
        }
        unsigned long long found = __ballot(member);
        while (found) {
          const int l = __builtin_ctzll(found);
          found &= found - 1;
#pragma unroll
          for (int q = 0; q < 3; ++q) c[q] += __shfl(xi[q], l);
          atoms += 1;
        }
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) c[q] /= (double)atoms;
      double spread = 0.0;
#pragma unroll 1
      for (int64_t base = a0; base < a1; base += WAVE) {
        const int64_t i = base + lane;
        const bool member = i < a1 && label[i] == root && bg_row(atom_row, i, M) >= 0;
        double d2 = 0.0;
        if (member) {
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const double d = x[i * 3 + q] - c[q];
            d2 += d * d;
          }
        }
        unsigned long long found = __ballot(member);
        while (found) {
          const int l = __builtin_ctzll(found);
          found &= found - 1;
          spread += __shfl(d2, l);
        }
      }
      const double rho = sqrt(spread / (double)atoms);
      if (!(rho > 0.0)) {                                            // all atoms in one point (or a NaN): not fitted
        for (int64_t i = a0 + tid; i < a1; i += TLS_THREADS) {
          const int64_t m = bg_row(atom_row, i, M);
          if (m >= 0 && label[i] == root) tls_blank(out, m, 0.0f, 0);
        }
        continue;
      }

      // ---- N = sum J_i^T J_i, b = sum J_i^T y_i, sum |y_i|^2
      double acc = 0.0;                                               // of this thread's entry of N, of b, or of |y|^2
#pragma unroll 1
      for (int64_t base = a0; base < a1; base += WAVE) {
        if (wid == 0) {
          const int64_t i = base + lane;
          const bool member = i < a1 && label[i] == root && bg_row(atom_row, i, M) >= 0;
          const unsigned long long found = __ballot(member);
          if (member) sh.members[__popcll(found & ((1ull << lane) - 1ull))] = lane;
          if (lane == 0) sh.count = __popcll(found);
        }
        __syncthreads();
        const int count = sh.count;
#pragma unroll 1
        for (int first = 0; first < count; first += TLS_STAGE) {
          const int staged = count - first < TLS_STAGE ? count - first : TLS_STAGE;
          if (tid < staged * TLS_ENTRIES) {
            const int at = tid / TLS_ENTRIES, e = tid - at * TLS_ENTRIES;
            const int64_t i = base + sh.members[first + at];
            if (e < 6 * TLS_P) {
              const int o = e / TLS_P, a = e - o * TLS_P;
              sh.j[at][o][a] = tls_design(o, a, (x[i * 3 + 0] - c[0]) / rho, (x[i * 3 + 1] - c[1]) / rho,
                                          (x[i * 3 + 2] - c[2]) / rho);
            } else {
              const int o = e - 6 * TLS_P, p = tls_p(o), q = tls_q(o);
              const int64_t m = bg_row(atom_row, i, M);
              const double s = 0.5 * ((double)u[m * 9 + p * 3 + q] + (double)u[m * 9 + q * 3 + p]);
              sh.y[at][o] = o < 3 ? s : TLS_SQRT2 * s;
            }
          }
          __syncthreads();
          if (tid < TLS_P * TLS_P) {
            const int a = tid / TLS_P, b = tid - a * TLS_P;
            for (int at = 0; at < staged; ++at) {
              double t = 0.0;
#pragma unroll
              for (int o = 0; o < 6; ++o) t += sh.j[at][o][a] * sh.j[at][o][b];
              acc += t;
            }
          } else if (tid < TLS_P * TLS_P + TLS_P) {
            const int a = tid - TLS_P * TLS_P;
            for (int at = 0; at < staged; ++at) {
              double t = 0.0;
#pragma unroll
              for (int o = 0; o < 6; ++o) t += sh.j[at][o][a] * sh.y[at][o];
              acc += t;
            }
          } else if (tid == TLS_P * TLS_P + TLS_P) {
            for (int at = 0; at < staged; ++at) {
              double t = 0.0;
#pragma unroll
              for (int o = 0; o < 6; ++o) t += sh.y[at][o] * sh.y[at][o];
              acc += t;
            }
          }
          __syncthreads();                                            // before the next stage
        }
        __syncthreads();                                              // every thread has read the count: the next list
      }
      if (tid < TLS_P * TLS_P) sh.n[tid] = acc;
      else if (tid < TLS_P * TLS_P + TLS_P) sh.b[tid - TLS_P * TLS_P] = acc;
      else if (tid == TLS_P * TLS_P + TLS_P) sh.sym2 = acc;
      __syncthreads();

      // ---- the eigen-decomposition and the minimum-norm solution
      const int sweeps = tls_jacobi(sh, TLS_P, tid);
      if (sweeps < 0) {
        const float nan = __builtin_nanf("");
        for (int64_t i = a0 + tid; i < a1; i += TLS_THREADS) {
          const int64_t m = bg_row(atom_row, i, M);
          if (m >= 0 && label[i] == root) tls_blank(out, m, nan, -1);
        }
        __syncthreads();
        continue;
      }
      if (tid < TLS_P) {
        double top = sh.n[0];
        for (int k = 1; k < TLS_P; ++k) top = fmax(top, sh.n[k * TLS_P + k]);
        const double lam = sh.n[tid * TLS_P + tid];
        double dot = 0.0;
        for (int a = 0; a < TLS_P; ++a) dot += sh.v[a * TLS_P + tid] * sh.b[a];
        sh.coef[tid] = lam > TLS_RANK_EPS * top ? dot / lam : 0.0;
        if (tid == 0) {
          int kept = 0;
          for (int k = 0; k < TLS_P; ++k) kept += sh.n[k * TLS_P + k] > TLS_RANK_EPS * top ? 1 : 0;
          sh.rank = kept;
        }
      }
      __syncthreads();
      if (tid < TLS_P) {
        double v = 0.0;
        for (int k = 0; k < TLS_P; ++k) v += sh.v[tid * TLS_P + k] * sh.coef[k];
        sh.p[tid] = v;
      }
      __syncthreads();
      if (tid < 9) {                                                  // T, L, S row-major, unscaled; c
        const int r = tid / 3, cidx = tid - r * 3;
        const int o = r == cidx ? r : 6 - r - cidx;                   // 12 -> 5, 13 -> 4, 23 -> 3
        sh.mol[tid] = sh.p[o];
        sh.mol[9 + tid] = sh.p[6 + o] / (rho * rho);
        // S's entry tid among its parameters 11 22 12 13 21 23 31 32; S33 = -(S11 + S22)
        const int k = tid == 0 ? 0 : (tid == 4 ? 1 : (tid < 4 ? tid + 1 : tid));
        sh.mol[18 + tid] = (tid == 8 ? -(sh.p[12] + sh.p[13]) : sh.p[12 + k]) / rho;
        if (tid < 3) sh.mol[27 + tid] = tid == 0 ? c[0] : (tid == 1 ? c[1] : c[2]);
      }
      __syncthreads();
      tls_principal(sh, 0, 0, tid);
      tls_principal(sh, 9, 3, tid);

      // ---- rows: u_tls and resid, one thread per member
      double r2 = 0.0;
      {
        double T[9], L[9], S[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          T[q] = sh.mol[q];
          L[q] = sh.mol[9 + q];
          S[q] = sh.mol[18 + q];
        }
#pragma unroll 1
        for (int64_t i = a0 + tid; i < a1; i += TLS_THREADS) {
          const int64_t m = bg_row(atom_row, i, M);
          if (m < 0 || label[i] != root) continue;
          const double rx = x[i * 3 + 0] - c[0], ry = x[i * 3 + 1] - c[1], rz = x[i * 3 + 2] - c[2];
          const double A[9] = {0.0, rz, -ry, -rz, 0.0, rx, ry, -rx, 0.0};
          double AL[9], AS[9], fit[9];
#pragma unroll
          for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              AL[p * 3 + q] = A[p * 3] * L[q] + A[p * 3 + 1] * L[3 + q] + A[p * 3 + 2] * L[6 + q];
              AS[p * 3 + q] = A[p * 3] * S[q] + A[p * 3 + 1] * S[3 + q] + A[p * 3 + 2] * S[6 + q];
            }
          }
          double d2 = 0.0;
#pragma unroll
          for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              const double ala = AL[p * 3] * A[q * 3] + AL[p * 3 + 1] * A[q * 3 + 1] + AL[p * 3 + 2] * A[q * 3 + 2];
              fit[p * 3 + q] = T[p * 3 + q] + ala + AS[p * 3 + q] + AS[q * 3 + p];
              const double s = 0.5 * ((double)u[m * 9 + p * 3 + q] + (double)u[m * 9 + q * 3 + p]);
              d2 += (s - fit[p * 3 + q]) * (s - fit[p * 3 + q]);
            }
          }
#pragma unroll
          for (int q = 0; q < 9; ++q) out.u_tls[m * 9 + q] = (float)fit[q];
          out.resid[m] = (float)sqrt(d2);
          r2 += d2;
        }
      }
      r2 = cr_wave_sum(r2);
      if (lane == 0) sh.fold[wid] = r2;
      __syncthreads();
      double total = sh.fold[0];
#pragma unroll
      for (int w = 1; w < TLS_WAVES; ++w) total += sh.fold[w];
      const double sym2 = sh.sym2;
      const float rfac = (float)(sym2 > 0.0 ? sqrt(total / sym2) : 0.0);
      const int32_t rank = sh.rank;

      // ---- the molecule's figures on every one of its rows
#pragma unroll 1
      for (int64_t i = a0 + tid; i < a1; i += TLS_THREADS) {
        const int64_t m = bg_row(atom_row, i, M);
        if (m < 0 || label[i] != root) continue;
        float* __restrict__ pr = out.params + m * 24;
        pr[0] = (float)sh.mol[0];  pr[1] = (float)sh.mol[4];   pr[2] = (float)sh.mol[8];
        pr[3] = (float)sh.mol[5];  pr[4] = (float)sh.mol[2];   pr[5] = (float)sh.mol[1];
        pr[6] = (float)sh.mol[9];  pr[7] = (float)sh.mol[13];  pr[8] = (float)sh.mol[17];
        pr[9] = (float)sh.mol[14]; pr[10] = (float)sh.mol[11]; pr[11] = (float)sh.mol[10];
#pragma unroll
        for (int q = 0; q < 12; ++q) pr[12 + q] = (float)sh.mol[18 + q];
#pragma unroll
        for (int q = 0; q < 6; ++q) out.eig[m * 6 + q] = (float)sh.eig[q];
        out.rank[m] = rank;
        out.rfac[m] = rfac;
      }
      __syncthreads();                                                // before the next molecule takes the LDS
    }
  }
}

__global__ __launch_bounds__(WAVE) void cn_tls_crystal_kernel(const float* __restrict__ u, const int64_t* __restrict__ label,
                                                              const int64_t* __restrict__ atom_row,
                                                              const int64_t* __restrict__ ptr, int64_t N, int64_t M,
                                                              const float* __restrict__ resid, const float* __restrict__ eig,
                                                              const int32_t* __restrict__ rank, double* __restrict__ stats) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t a0, a1;
  cr_rows(ptr, g, N, a0, a1);
  double fitted = 0.0, deficient = 0.0, negative = 0.0, r2 = 0.0, s2 = 0.0, hi = 0.0;
  for (int64_t i = a0 + lane; i < a1; i += WAVE) {
    const int64_t m = bg_row(atom_row, i, M);
    if (m < 0) continue;
    const int32_t rk = rank[m];
    if (rk == 0) continue;
    if (label[i] == i) {
      fitted += 1.0;
      deficient += rk < TLS_P ? 1.0 : 0.0;
      negative += (eig[m * 6] < 0.0f || eig[m * 6 + 3] < 0.0f) ? 1.0 : 0.0;
    }
    const double r = (double)resid[m];
    r2 += r * r;
    hi = cr_max_nan(hi, r);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double s = 0.5 * ((double)u[m * 9 + p * 3 + q] + (double)u[m * 9 + q * 3 + p]);
        s2 += s * s;
      }
    }
  }
  fitted = cr_wave_sum(fitted);
  deficient = cr_wave_sum(deficient);
  negative = cr_wave_sum(negative);
  r2 = cr_wave_sum(r2);
  s2 = cr_wave_sum(s2);
  hi = cr_wave_max_nan(hi);
  if (lane == 0) {
    double* __restrict__ s = stats + (size_t)g * 6;
    s[0] = fitted;
    s[1] = deficient;
    s[2] = negative;
    s[3] = r2;
    s[4] = s2;
    s[5] = hi;
  }
}

}  // namespace

extern "C" int cartnet_adp_tls_fit(const float* u, const int64_t* label, const double* x, const int64_t* atom_row,
                                   const int64_t* ptr, const int64_t* row_ptr, const int32_t* mol_status,
                                   const int32_t* mol_size, int32_t B, int64_t N, int64_t M, float* u_tls, float* resid,
                                   float* params, float* eig, int32_t* rank, float* rfac, double* crystal_stats,
                                   void* stream) {
  CN_CHECK(B >= 0 && N >= 0 && M >= 0, "cartnet_adp_tls_fit: bad sizes (B=%d, N=%lld, M=%lld)", B, (long long)N,
           (long long)M);
  if (M == 0 || B == 0 || N == 0) return 0;
  CN_CHECK(u && label && x && atom_row && ptr && row_ptr && mol_status && mol_size && u_tls && resid && params && eig &&
               rank && rfac,
           "cartnet_adp_tls_fit: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const TlsOut out = {u_tls, resid, params, eig, rank, rfac};
  hipLaunchKernelGGL(cn_tls_fit_kernel, dim3((unsigned)B, TLS_SLOTS), dim3(TLS_THREADS), 0, st, u, label, x, atom_row, ptr,
                     mol_status, mol_size, N, M, out);
  CN_LAUNCH_CHECK("cartnet_adp_tls_fit");
  if (crystal_stats) {
    hipLaunchKernelGGL(cn_tls_crystal_kernel, dim3((unsigned)B), dim3(WAVE), 0, st, u, label, atom_row, ptr, N, M, resid,
                       eig, rank, crystal_stats);
    CN_LAUNCH_CHECK("cartnet_adp_tls_fit");
  }
  return 0;
}
