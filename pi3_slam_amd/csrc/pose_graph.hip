// A Sim(3) pose graph over the chunks of a sequence (loop closure, loop_closure.py), f64, on the device.
//
// Node c: W_c, the 4x4 similarity (row-major) that takes chunk c to the world.  Edge e = (i, j): a measured relative
// similarity Z_e (chunk j's frame -> chunk i's), a centre c_e in chunk i's frame and a symmetric 7x7 information matrix
// O_e (its upper triangle row-major, as pi3_cloud_pair_equations writes A).
//   chart(E, c) = (w, l, t) for E = [sR | tau]:  w = the rotation vector of R, l = ln s, t = tau - c + sR c
//                 (the inverse of map_eval.sim3_increment(x, c); parameter order w (3), l, t (3))
//   r_e = chart(W_i^-1 W_j Z_e^-1, c_e),   F = sum_e r_e^T O_e r_e
// Levenberg-Marquardt over the free nodes: the step of node k is d_k in R^7, W_k <- inc(d_k, g_k) W_k with
// inc(x, g) = [ e^l exp([w]x) | g + t - e^l exp([w]x) g ] and g_k the caller's centre of node k (fixed for the solve).
//
// Jacobians (analytic, at d = 0).  With Ai = W_i^-1, B = W_j Z^-1 and G_k(g) = d inc / d x_k at 0 = [ L_k | t_k - L_k g ]
// (L_k = [e_k]x for w, I for l, 0 for t; t_k = e_(k-4) for t):   dE = +Ai G_k(g_j) B for node j,  -Ai G_k(g_i) B for
// node i.  With M = E's 3x3, q = sum M^2, s = sqrt(q / 3), R = M / s:
//   dl = sum(M . dM) / q;   dR = dM / s - R dl;   omega = vee(skew part of dR R^T);
//   dw = omega - (w x omega) / 2 + kappa w x (w x omega),  kappa = 1 / th^2 - (1 + cos th) / (2 th sin th)
//        (the inverse left Jacobian of SO(3); th < 1e-4: kappa = 1 / 12 + th^2 / 720);
//   dt = dtau + dM c.
// Normal equations (dense, n = 7 C): H = sum J^T O J, g = sum J^T O r.  One workgroup per node writes that node's block
// row, walking the edges in index order, every entry owned by one thread: no floating-point atomics, the same bits
// every run.  A fixed node, and a free node without a (valid) edge, keeps identity rows and a zero right-hand side.
// An edge with an index outside [0, C) or with i == j is left out of the cost and of the equations.
//   (H + lambda diag H) d = -g by a blocked right-looking Cholesky (32 columns per step: the diagonal block in LDS by
//   one workgroup, the panel below it a row per thread, the trailing update an entry per thread), then the two
//   triangular solves by one workgroup.  Nothing about its speed has been measured beyond "it is not what the solve
//   waits for at tens of chunks".
// One iteration (tests/loop_closure_ref.py states the same steps in numpy):
//   factor; a failure (a pivot that is not positive and finite): lambda >= 1e12 -> status 2, else lambda *= 10;
//   F' = F(candidate);  max |d| < 1e-9 -> converged, and that last step is applied when F' is finite;
//   |F - F'| <= 1e-12 F -> converged (F no longer moves; that last step is applied, whichever way the difference rounds);
//   F' < F: accept, lambda = max(lambda / 10, 1e-12);
//   otherwise lambda = min(10 lambda, 1e12).
// The decision and lambda live in a device state block; the host launches max_iterations rounds of the same kernels
// and a round returns at once when the solve is over (as csrc/ba.hip does).  lambda starts at 1e-4.
#include "common.h"

namespace {

constexpr int kMaxNodes = 448;
constexpr int kEdgeDoubles = 210;        // r 7 | Ji 49 | Jj 49 | O Ji 49 | O Jj 49 | O r 7
constexpr int kNb = 32;                  // columns per Cholesky step
constexpr double kLambda0 = 1e-4, kLambdaMin = 1e-12, kLambdaMax = 1e12, kStepTol = 1e-9, kCostTol = 1e-12;

struct PgState {
  double cost, lambda, iters, accepted, status, done, chol_fail, step, initial_cost, accept;
};

struct PgGraph {
  const int* edges;            // [E][2]
  const double* Z;             // [E][16]
  const double* ecentres;      // [E][3]
  const double* info;          // [E][28]
  const double* centres;       // [C][3]
  int C, E;
};

// ---- 3x4 similarities [A | tau] (row-major 12 doubles; the fourth row 0 0 0 1 is implied)
__device__ __forceinline__ void sim_load(const double* __restrict__ M16, double m[12]) {
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = M16[k];
}
__device__ __forceinline__ void sim_mul(const double a[12], const double b[12], double o[12]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      o[4 * r + c] = (a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c]) + a[4 * r + 2] * b[8 + c] + (c == 3 ? a[4 * r + 3] : 0.0);
  }
}
// A^-1 = A^T / s^2 with s^2 = sum A^2 / 3;  tau' = -A^-1 tau
__device__ __forceinline__ void sim_inv(const double a[12], double o[12]) {
  double q = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) q += a[4 * r + c] * a[4 * r + c];
  const double is2 = 3.0 / q;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[4 * r + c] = a[4 * c + r] * is2;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) o[4 * r + 3] = -((o[4 * r] * a[3] + o[4 * r + 1] * a[7]) + o[4 * r + 2] * a[11]);
}

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// inc(x, g): x = (w, l, t)
__device__ __forceinline__ void sim_increment(const double x[7], const double g[3], double o[12]) {
  const double th = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (th > 0.0) {
    const double k0 = x[0] / th, k1 = x[1] / th, k2 = x[2] / th;
    const double K[9] = {0.0, -k2, k1, k2, 0.0, -k0, -k1, k0, 0.0};
    const double sn = sin(th), cs = 1.0 - cos(th);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double kk = (K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c]) + K[3 * r + 2] * K[6 + c];
        R[3 * r + c] += sn * K[3 * r + c] + cs * kk;
      }
  }
  const double s = exp(x[3]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[4 * r + c] = s * R[3 * r + c];
    o[4 * r + 3] = (g[r] + x[4 + r]) - ((o[4 * r] * g[0] + o[4 * r + 1] * g[1]) + o[4 * r + 2] * g[2]);
  }
}

// chart(E, c) -> x (7); also s and R for the Jacobians
__device__ __forceinline__ void sim_chart(const double E[12], const double c[3], double x[7], double& s, double R[9]) {
  double q = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) q += E[4 * r + k] * E[4 * r + k];
  s = sqrt(q / 3.0);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) R[3 * r + k] = E[4 * r + k] / s;
  const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double nv = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double th = atan2(0.5 * nv, 0.5 * (((R[0] + R[4]) + R[8]) - 1.0));
  const double f = nv < 1e-12 ? 0.5 : th / nv;
  x[0] = f * v[0], x[1] = f * v[1], x[2] = f * v[2];
  x[3] = log(s);
#pragma unroll
  for (int r = 0; r < 3; ++r)
    x[4 + r] = (E[4 * r + 3] - c[r]) + ((E[4 * r] * c[0] + E[4 * r + 1] * c[1]) + E[4 * r + 2] * c[2]);
}

__device__ __forceinline__ bool edge_nodes(const PgGraph& gr, int e, int& i, int& j) {
  i = gr.edges[2 * e], j = gr.edges[2 * e + 1];
  return i >= 0 && i < gr.C && j >= 0 && j < gr.C && i != j;
}

// O v for the packed upper triangle
__device__ __forceinline__ void info_mul(const double* __restrict__ U, const double v[7], double o[7]) {
  double O[7][7];
  int t = 0;
#pragma unroll
  for (int a = 0; a < 7; ++a)
#pragma unroll
    for (int b = a; b < 7; ++b) O[a][b] = O[b][a] = U[t++];
#pragma unroll
  for (int a = 0; a < 7; ++a) {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 7; ++b) acc += O[a][b] * v[b];
    o[a] = acc;
  }
}

// the residual of edge e at `nodes`; Ai = W_i^-1, B = W_j Z^-1, E = Ai B for the caller that goes on
__device__ __forceinline__ void edge_residual(const PgGraph& gr, const double* __restrict__ nodes, int e, int i, int j,
                                              double Ai[12], double B[12], double E[12], double x[7], double& s,
                                              double R[9]) {
  double Wi[12], Wj[12], Zm[12], Zi[12];
  sim_load(nodes + 16 * i, Wi);
  sim_load(nodes + 16 * j, Wj);
  sim_load(gr.Z + 16L * e, Zm);
  sim_inv(Wi, Ai);
  sim_inv(Zm, Zi);
  sim_mul(Wj, Zi, B);
  sim_mul(Ai, B, E);
  sim_chart(E, gr.ecentres + 3L * e, x, s, R);
}

// cost_e[e] = r^T O r at `nodes` (0 for an edge that is left out)
__global__ __launch_bounds__(64) void pg_cost_kernel(PgGraph gr, const double* __restrict__ nodes,
                                                     double* __restrict__ cost_e, const PgState* st, int candidate) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= gr.E || st->done != 0.0 || (candidate && st->chol_fail != 0.0)) return;
  int i, j;
  double c = 0.0;
  if (edge_nodes(gr, e, i, j)) {
    double Ai[12], B[12], E[12], x[7], s, R[9], ox[7];
    edge_residual(gr, nodes, e, i, j, Ai, B, E, x, s, R);
    info_mul(gr.info + 28L * e, x, ox);
#pragma unroll
    for (int a = 0; a < 7; ++a) c += x[a] * ox[a];
  }
  cost_e[e] = c;
}

// column k of d chart for dE = sign Ai G_k(g) B
__device__ __forceinline__ void chart_column(int k, double sign, const double Ai[12], const double B[12], const double g[3],
                                             const double E[12], const double x[7], double s, const double R[9],
                                             const double c[3], double col[7]) {
  // G = [ L | u ],  u = t_k - L g
  double L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, u[3] = {0, 0, 0};
  if (k < 3) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;      // [e_k]x: entry (b, a) = 1, (a, b) = -1
    L[3 * b + a] = 1.0;
    L[3 * a + b] = -1.0;
  } else if (k == 3) {
    L[0] = L[4] = L[8] = 1.0;
  } else {
    u[k - 4] = 1.0;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) u[r] -= (L[3 * r] * g[0] + L[3 * r + 1] * g[1]) + L[3 * r + 2] * g[2];
  // X = Ai3 L (3x3), x4 = Ai3 u;  dE = sign [ X B3 | X B_tau + x4 ]
  double X[9], x4[3], dE[12];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int q = 0; q < 3; ++q) X[3 * r + q] = (Ai[4 * r] * L[q] + Ai[4 * r + 1] * L[3 + q]) + Ai[4 * r + 2] * L[6 + q];
    x4[r] = (Ai[4 * r] * u[0] + Ai[4 * r + 1] * u[1]) + Ai[4 * r + 2] * u[2];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      dE[4 * r + q] = sign * (((X[3 * r] * B[q] + X[3 * r + 1] * B[4 + q]) + X[3 * r + 2] * B[8 + q]) + (q == 3 ? x4[r] : 0.0));
  double md = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) md += E[4 * r + q] * dE[4 * r + q];
  const double dl = md / (3.0 * s * s);
  double dR[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) dR[3 * r + q] = dE[4 * r + q] / s - R[3 * r + q] * dl;
  double Om[9];                                      // dR R^T
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) Om[3 * r + q] = (dR[3 * r] * R[3 * q] + dR[3 * r + 1] * R[3 * q + 1]) + dR[3 * r + 2] * R[3 * q + 2];
  const double om[3] = {0.5 * (Om[7] - Om[5]), 0.5 * (Om[2] - Om[6]), 0.5 * (Om[3] - Om[1])};
  const double w[3] = {x[0], x[1], x[2]};
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(th2);
  const double kappa = th < 1e-4 ? 1.0 / 12.0 + th2 / 720.0 : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
  double wo[3], wwo[3];
  cross3(w, om, wo);
  cross3(w, wo, wwo);
#pragma unroll
  for (int r = 0; r < 3; ++r) col[r] = (om[r] - 0.5 * wo[r]) + kappa * wwo[r];
  col[3] = dl;
#pragma unroll
  for (int r = 0; r < 3; ++r) col[4 + r] = dE[4 * r + 3] + ((dE[4 * r] * c[0] + dE[4 * r + 1] * c[1]) + dE[4 * r + 2] * c[2]);
}

// per edge: r, Ji, Jj (7x7 row-major: row = residual component, column = parameter), O Ji, O Jj, O r
__global__ __launch_bounds__(64) void pg_linearize_kernel(PgGraph gr, const double* __restrict__ nodes,
                                                          double* __restrict__ edata, const PgState* st) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= gr.E || st->done != 0.0) return;
  int i, j;
  if (!edge_nodes(gr, e, i, j)) return;
  double* __restrict__ d = edata + (long)kEdgeDoubles * e;
  double Ai[12], B[12], E[12], x[7], s, R[9], o[7];
  edge_residual(gr, nodes, e, i, j, Ai, B, E, x, s, R);
  const double* c = gr.ecentres + 3L * e;
  const double* U = gr.info + 28L * e;
#pragma unroll
  for (int a = 0; a < 7; ++a) d[a] = x[a];
  info_mul(U, x, o);
#pragma unroll
  for (int a = 0; a < 7; ++a) d[203 + a] = o[a];
  for (int side = 0; side < 2; ++side) {
    const double* g = gr.centres + 3 * (side ? j : i);
    const double gg[3] = {g[0], g[1], g[2]};
    double* J = d + 7 + 49 * side;
    double* OJ = d + 105 + 49 * side;
    for (int k = 0; k < 7; ++k) {
      double col[7];
      chart_column(k, side ? 1.0 : -1.0, Ai, B, gg, E, x, s, R, c, col);
      info_mul(U, col, o);
#pragma unroll
      for (int a = 0; a < 7; ++a) {
        J[7 * a + k] = col[a];
        OJ[7 * a + k] = o[a];
      }
    }
  }
}

// active[k] = 1 when node k is free and has a valid edge
__global__ __launch_bounds__(64) void pg_active_kernel(PgGraph gr, const unsigned char* __restrict__ fixed,
                                                       double* __restrict__ active) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= gr.C) return;
  int deg = 0;
  for (int e = 0; e < gr.E; ++e) {
    int i, j;
    if (edge_nodes(gr, e, i, j) && (i == k || j == k)) ++deg;
  }
  active[k] = (!fixed[k] && deg > 0) ? 1.0 : 0.0;
}

// block row k of H + lambda diag H (all n columns) and of -g.  Threads 0..48: the diagonal block, entry (a, b), in a
// register; 64..112: the block against the edge's other node, read-modify-write in global memory, one thread per
// address; 128..134: g.  Edges in index order.
__global__ __launch_bounds__(256) void pg_assemble_kernel(PgGraph gr, const double* __restrict__ edata,
                                                          const double* __restrict__ active, double* __restrict__ H,
                                                          double* __restrict__ rhs, const PgState* st) {
  if (st->done != 0.0) return;
  const int k = blockIdx.x, tid = (int)threadIdx.x;
  const long n = 7L * gr.C;
  double* __restrict__ row = H + 7L * k * n;
  for (long q = tid; q < 7 * n; q += 256) row[q] = 0.0;
  __syncthreads();
  const bool on = active[k] != 0.0;
  const int grp = tid >> 6, loc = tid & 63;
  const int a = loc / 7, b = loc - 7 * a;
  double acc = 0.0;
  if (on) {
    for (int e = 0; e < gr.E; ++e) {
      int i, j;
      if (!edge_nodes(gr, e, i, j) || (i != k && j != k)) continue;
      const double* __restrict__ d = edata + (long)kEdgeDoubles * e;
      const int mine = i == k ? 0 : 1, other = i == k ? j : i;
      const double* Jm = d + 7 + 49 * mine;
      if (grp == 0 && loc < 49) {
        const double* OJ = d + 105 + 49 * mine;
#pragma unroll
        for (int c = 0; c < 7; ++c) acc += Jm[7 * c + a] * OJ[7 * c + b];
      } else if (grp == 1 && loc < 49 && active[other] != 0.0) {
        const double* OJ = d + 105 + 49 * (1 - mine);
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < 7; ++c) v += Jm[7 * c + a] * OJ[7 * c + b];
        row[a * n + 7 * other + b] += v;
      } else if (grp == 2 && loc < 7) {
#pragma unroll
        for (int c = 0; c < 7; ++c) acc += Jm[7 * c + loc] * d[203 + c];
      }
    }
  }
  if (grp == 0 && loc < 49) row[a * n + 7 * k + b] = on ? (a == b ? acc * (1.0 + st->lambda) : acc) : (a == b ? 1.0 : 0.0);
  if (grp == 2 && loc < 7) rhs[7 * k + loc] = on ? -acc : 0.0;
}

// ---- Cholesky of the lower triangle of H (n x n, row-major), in place, 32 columns per step
__global__ __launch_bounds__(256) void pg_chol_diag_kernel(double* __restrict__ H, long n, long k0, int nb, PgState* st) {
  __shared__ double S[kNb][kNb + 1];
  __shared__ int bad;
  if (st->done != 0.0 || st->chol_fail != 0.0) return;
  const int tid = (int)threadIdx.x;
  for (int q = tid; q < nb * nb; q += 256) S[q / nb][q % nb] = H[(k0 + q / nb) * n + k0 + q % nb];
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int p = 0; p < nb; ++p) {
    const double dgn = S[p][p];
    if (!(dgn > 0.0 && dgn < __builtin_inf())) {     // the same value in every thread
      if (tid == 0) bad = 1;
      break;
    }
    const double l = sqrt(dgn);
    __syncthreads();
    if (tid == 0) S[p][p] = l;
    for (int r = p + 1 + tid; r < nb; r += 256) S[r][p] /= l;
    __syncthreads();
    for (int q = tid; q < nb * nb; q += 256) {
      const int r = q / nb, c = q % nb;
      if (c > p && r >= c) S[r][c] -= S[r][p] * S[c][p];
    }
    __syncthreads();
  }
  __syncthreads();
  if (bad) {
    if (tid == 0) st->chol_fail = 1.0;
    return;
  }
  for (int q = tid; q < nb * nb; q += 256)
    if (q / nb >= q % nb) H[(k0 + q / nb) * n + k0 + q % nb] = S[q / nb][q % nb];
}

// the panel below the diagonal block: row r, L[r][k0 + c] = (A[r][k0 + c] - sum_{p < c} L[r][k0 + p] D[c][p]) / D[c][c]
__global__ __launch_bounds__(256) void pg_chol_panel_kernel(double* __restrict__ H, long n, long k0, int nb,
                                                            const PgState* st) {
  __shared__ double D[kNb][kNb + 1];
  if (st->done != 0.0 || st->chol_fail != 0.0) return;
  const int tid = (int)threadIdx.x;
  for (int q = tid; q < nb * nb; q += 256) D[q / nb][q % nb] = H[(k0 + q / nb) * n + k0 + q % nb];
  __syncthreads();
  const long r = k0 + nb + (long)blockIdx.x * 256 + tid;
  if (r >= n) return;
  double* __restrict__ x = H + r * n + k0;
  for (int c = 0; c < nb; ++c) {
    double v = x[c];
    for (int p = 0; p < c; ++p) v -= x[p] * D[c][p];
    x[c] = v / D[c][c];
  }
}

// the trailing update: A[r][c] -= sum_p L[r][k0 + p] L[c][k0 + p] for r >= c >= k0 + nb
__global__ __launch_bounds__(256) void pg_chol_update_kernel(double* __restrict__ H, long n, long k0, int nb,
                                                             const PgState* st) {
  if (st->done != 0.0 || st->chol_fail != 0.0) return;
  if (blockIdx.x > blockIdx.y) return;              // a tile above the diagonal
  const long t0 = k0 + nb;
  const long c = t0 + 16L * blockIdx.x + (threadIdx.x & 15), r = t0 + 16L * blockIdx.y + (threadIdx.x >> 4);
  if (r >= n || c > r) return;
  const double* __restrict__ lr = H + r * n + k0;
  const double* __restrict__ lc = H + c * n + k0;
  double v = 0.0;
  for (int p = 0; p < nb; ++p) v += lr[p] * lc[p];
  H[r * n + c] -= v;
}

// L y = rhs, L^T d = y by one workgroup; st->step = max |d|
__global__ __launch_bounds__(256) void pg_solve_kernel(const double* __restrict__ L, long n, const double* __restrict__ rhs,
                                                       double* __restrict__ delta, PgState* st) {
  __shared__ double y[7 * kMaxNodes];
  if (st->done != 0.0 || st->chol_fail != 0.0) return;
  const int tid = (int)threadIdx.x;
  for (long q = tid; q < n; q += 256) y[q] = rhs[q];
  for (long k = 0; k < n; ++k) {
    __syncthreads();
    const double yk = y[k] / L[k * n + k];
    __syncthreads();
    if (tid == 0) y[k] = yk;
    for (long r = k + 1 + tid; r < n; r += 256) y[r] -= L[r * n + k] * yk;
  }
  for (long k = n - 1; k >= 0; --k) {
    __syncthreads();
    const double xk = y[k] / L[k * n + k];
    __syncthreads();
    if (tid == 0) y[k] = xk;
    for (long c = tid; c < k; c += 256) y[c] -= L[k * n + c] * xk;
  }
  __syncthreads();
  for (long q = tid; q < n; q += 256) delta[q] = y[q];
  if (tid == 0) {
    double m = 0.0;
    bool finite = true;
    for (long q = 0; q < n; ++q) {
      const double v = fabs(y[q]);
      finite = finite && v < __builtin_inf();
      m = v > m ? v : m;
    }
    st->step = finite ? m : __builtin_nan("");
  }
}

__global__ __launch_bounds__(64) void pg_candidate_kernel(PgGraph gr, const double* __restrict__ nodes,
                                                          const double* __restrict__ active,
                                                          const double* __restrict__ delta, double* __restrict__ nodes_new,
                                                          const PgState* st) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= gr.C || st->done != 0.0 || st->chol_fail != 0.0) return;
  const double* W = nodes + 16 * k;
  double* out = nodes_new + 16 * k;
  if (active[k] == 0.0) {
    for (int q = 0; q < 16; ++q) out[q] = W[q];
    return;
  }
  double x[7], D[12], Wm[12], o[12];
  for (int q = 0; q < 7; ++q) x[q] = delta[7 * k + q];
  const double g[3] = {gr.centres[3 * k], gr.centres[3 * k + 1], gr.centres[3 * k + 2]};
  sim_increment(x, g, D);
  sim_load(W, Wm);
  sim_mul(D, Wm, o);
  for (int q = 0; q < 12; ++q) out[q] = o[q];
  out[12] = 0.0, out[13] = 0.0, out[14] = 0.0, out[15] = 1.0;
}

// the sum of the edges' costs in index order (thread 0)
__device__ __forceinline__ double pg_total(const double* __restrict__ cost_e, int E) {
  double s = 0.0;
  for (int e = 0; e < E; ++e) s += cost_e[e];
  return s;
}

__global__ void pg_init_kernel(const double* __restrict__ cost_e, int E, PgState* st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double c = pg_total(cost_e, E);
  st->cost = c, st->initial_cost = c, st->lambda = kLambda0, st->iters = 0.0, st->accepted = 0.0, st->status = 1.0;
  st->done = 0.0, st->chol_fail = 0.0, st->step = 0.0, st->accept = 0.0;
}

__global__ __launch_bounds__(256) void pg_decide_kernel(const double* __restrict__ cost_e, int E, int C,
                                                        double* __restrict__ nodes, const double* __restrict__ nodes_new,
                                                        PgState* st) {
  __shared__ int take;
  if (st->done != 0.0) return;
  const int tid = (int)threadIdx.x;
  if (tid == 0) {
    take = 0;
    st->iters += 1.0;
    if (st->chol_fail != 0.0 || !(st->step == st->step)) {
      st->chol_fail = 0.0;
      if (st->lambda >= kLambdaMax) st->status = 2.0, st->done = 1.0;
      else st->lambda = fmin(st->lambda * 10.0, kLambdaMax);
    } else if (st->step < kStepTol) {
      const double fn = pg_total(cost_e, E);
      st->status = 0.0, st->done = 1.0;
      if (fn >= 0.0 && fn < __builtin_inf()) st->cost = fn, st->accepted += 1.0, take = 1;
    } else {
      const double fn = pg_total(cost_e, E);
      const double dec = st->cost - fn;              // (NaN compares false below: a rejection)
      if (fabs(dec) <= kCostTol * st->cost) {        // F no longer moves: the last step is applied, whichever way
        st->status = 0.0, st->done = 1.0;            // the difference rounds
        st->cost = fn, st->accepted += 1.0, take = 1;
      } else if (dec > 0.0) {
        st->cost = fn;
        st->accepted += 1.0;
        st->lambda = fmax(st->lambda / 10.0, kLambdaMin);
        take = 1;
      } else {
        st->lambda = fmin(st->lambda * 10.0, kLambdaMax);
      }
    }
  }
  __syncthreads();
  if (take)
    for (int q = tid; q < 16 * C; q += 256) nodes[q] = nodes_new[q];
}

__global__ __launch_bounds__(256) void pg_finish_kernel(int C, double* __restrict__ nodes, const double* __restrict__ nodes_in,
                                                        const PgState* st, double* __restrict__ out) {
  const int tid = (int)threadIdx.x;
  if (st->status == 2.0)
    for (int q = tid; q < 16 * C; q += 256) nodes[q] = nodes_in[q];
  if (tid < 16) {
    const double v[6] = {st->cost, st->initial_cost, st->iters, st->accepted, st->lambda, st->status};
    out[tid] = tid < 6 ? v[tid] : 0.0;
  }
}

struct PgLayout {
  long state, nodes_in, nodes_new, active, edata, cost_e, H, rhs, delta, total;
};
inline PgLayout pg_layout(int C, int E) {
  PgLayout l;
  const long n = 7L * C;
  long at = 0;
  l.state = at, at += 16;
  l.nodes_in = at, at += 16L * C;
  l.nodes_new = at, at += 16L * C;
  l.active = at, at += C;
  l.edata = at, at += (long)kEdgeDoubles * E;
  l.cost_e = at, at += E;
  l.H = at, at += n * n;
  l.rhs = at, at += n;
  l.delta = at, at += n;
  l.total = at;
  return l;
}

}  // namespace

extern "C" int pi3_pose_graph_workspace(int C, int E, long* doubles) {
  if (C < 1 || C > kMaxNodes || E < 0 || !doubles) {
    pi3_set_error("pi3_pose_graph_workspace: bad arguments C=%d (1 .. %d) E=%d (>= 0), or a null pointer", C, kMaxNodes, E);
    return PI3_ERR_ARG;
  }
  *doubles = pg_layout(C, E).total;
  return PI3_OK;
}

extern "C" int pi3_pose_graph_sim3(double* nodes, const double* centres, int C, const int* edges, const double* Z,
                                   const double* edge_centres, const double* info, int E, const unsigned char* fixed,
                                   int max_iterations, double* workspace, long workspace_doubles, double* out,
                                   void* stream) {
  if (C < 1 || C > kMaxNodes || E < 0 || max_iterations < 0 || !nodes || !centres || !fixed || !workspace || !out ||
      (E > 0 && (!edges || !Z || !edge_centres || !info))) {
    pi3_set_error("pi3_pose_graph_sim3: bad arguments C=%d (1 .. %d) E=%d (>= 0) max_iterations=%d (>= 0), or a null "
                  "pointer", C, kMaxNodes, E, max_iterations);
    return PI3_ERR_ARG;
  }
  const PgLayout l = pg_layout(C, E);
  if (workspace_doubles < l.total) {
    pi3_set_error("pi3_pose_graph_sim3: C=%d E=%d needs %ld doubles of workspace, the caller has %ld", C, E, l.total,
                  workspace_doubles);
    return PI3_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  PgState* st = (PgState*)(workspace + l.state);
  double* nodes_in = workspace + l.nodes_in;
  double* nodes_new = workspace + l.nodes_new;
  double* active = workspace + l.active;
  double* edata = workspace + l.edata;
  double* cost_e = workspace + l.cost_e;
  double* H = workspace + l.H;
  double* rhs = workspace + l.rhs;
  double* delta = workspace + l.delta;
  const PgGraph gr = {edges, Z, edge_centres, info, centres, C, E};
  const long n = 7L * C;
  const dim3 per_edge((unsigned)((E + 63) / 64 > 0 ? (E + 63) / 64 : 1)), per_node((unsigned)((C + 63) / 64)), b64(64), b256(256);
  if (hipMemcpyAsync(nodes_in, nodes, sizeof(double) * 16 * C, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemsetAsync(st, 0, sizeof(double) * 16, s) != hipSuccess) {
    pi3_set_error("pi3_pose_graph_sim3: the copy of the input nodes failed");
    return PI3_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(pg_active_kernel, per_node, b64, 0, s, gr, fixed, active);
  hipLaunchKernelGGL(pg_cost_kernel, per_edge, b64, 0, s, gr, (const double*)nodes, cost_e, (const PgState*)st, 0);
  hipLaunchKernelGGL(pg_init_kernel, dim3(1), b64, 0, s, (const double*)cost_e, E, st);
  for (int it = 0; it < max_iterations; ++it) {
    hipLaunchKernelGGL(pg_linearize_kernel, per_edge, b64, 0, s, gr, (const double*)nodes, edata, (const PgState*)st);
    hipLaunchKernelGGL(pg_assemble_kernel, dim3((unsigned)C), b256, 0, s, gr, (const double*)edata, (const double*)active,
                       H, rhs, (const PgState*)st);
    for (long k0 = 0; k0 < n; k0 += kNb) {
      const int nb = (int)(n - k0 < kNb ? n - k0 : kNb);
      const long below = n - k0 - nb;
      hipLaunchKernelGGL(pg_chol_diag_kernel, dim3(1), b256, 0, s, H, n, k0, nb, st);
      if (below > 0) {
        hipLaunchKernelGGL(pg_chol_panel_kernel, dim3((unsigned)((below + 255) / 256)), b256, 0, s, H, n, k0, nb,
                           (const PgState*)st);
        const unsigned tiles = (unsigned)((below + 15) / 16);
        hipLaunchKernelGGL(pg_chol_update_kernel, dim3(tiles, tiles), b256, 0, s, H, n, k0, nb, (const PgState*)st);
      }
    }
    hipLaunchKernelGGL(pg_solve_kernel, dim3(1), b256, 0, s, (const double*)H, n, (const double*)rhs, delta, st);
    hipLaunchKernelGGL(pg_candidate_kernel, per_node, b64, 0, s, gr, (const double*)nodes, (const double*)active,
                       (const double*)delta, nodes_new, (const PgState*)st);
    hipLaunchKernelGGL(pg_cost_kernel, per_edge, b64, 0, s, gr, (const double*)nodes_new, cost_e, (const PgState*)st, 1);
    hipLaunchKernelGGL(pg_decide_kernel, dim3(1), b256, 0, s, (const double*)cost_e, E, C, nodes,
                       (const double*)nodes_new, st);
  }
  hipLaunchKernelGGL(pg_finish_kernel, dim3(1), b256, 0, s, C, nodes, (const double*)nodes_in, (const PgState*)st, out);
  return pi3_check_launch("pose_graph_sim3");
}
