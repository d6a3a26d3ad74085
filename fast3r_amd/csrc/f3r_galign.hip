// Global alignment (PointCloudOptimizer.forward, fast3r/dust3r/cloud_opt/optimizer.py:219-266, with l1_dist / l2_dist of commons.py): the
// loss and every gradient it has, at the level of matrices, in one evaluation.
//   d = exp(l_v[p]);  q = (d (x - cx) / f, d (y - cy) / f, d);  X = R_v q + t_v
//   A = S_e (a_e * P_o[p]) + m_e;  r = X - A;  cost = w_o[p] |r| (l1) or w_o[p] |r|^2 (l2);  loss = sum_o k_o sum_p cost
// A pixel of a view has one owner.  Workgroup (slot, v) owns the chunks slot, slot + S_v, .. of view v (GA_CHUNK pixels each, GA_PPT per
// thread); per chunk it walks the view's observation list once, keeps G = sum_o g of its pixels in registers and writes dL/dl once.
//   * per (observation, chunk) 12 sums -- Q = sum g P^T and sum g -- go through block_sum and are added to the row (observation, slot) of the
//     workspace by the thread that owns the word: the same thread, the same chunks, the same order in every run, no atomic.  dL/dS, dL/dm
//     and dL/da all follow from them: sum g (a * P)^T = Q diag(a), and sum (S^T g) * P has the entries sum_i S_ic Q_ic;
//   * per workgroup the 16 sums of the view (dL/dR, dL/dt, dL/df, dL/dc, the loss) go through one block_sum into the row (view, slot);
//   * galign_finish_kernel adds the rows in slot order (side 0 before side 1 for an edge), forms the edge gradients and rounds to fp32;
//     galign_loss_kernel adds the views' losses in a fixed order.  Two runs give the same bits.
// The arithmetic is fp64 on the exactly widened fp32 inputs (docs/rows_f.md "global alignment" says why); the workspace holds GA_SLOTS rows
// per view and per observation whatever the image size.  Edge constants are read through wave-uniform addresses.
#include "f3r_common.h"

#include <cmath>
#include <cstddef>

#include "f3r_prims.h"

// build.sh compiles this file with -ffp-contract=off: every product and sum below is rounded on its own, in the order written, as
// tests/galign_ref.py writes them as separate tensor operations.

namespace {

constexpr int GA_NT = 256;                      // threads of a workgroup
constexpr int GA_PPT = 2;                       // pixels of a chunk per thread (4: 256 VGPRs and one wave per SIMD, 2 - 18 % slower)
constexpr int GA_CHUNK = GA_NT * GA_PPT;        // pixels of a chunk
constexpr int GA_SLOTS = 64;                    // workgroups, and partial rows, per view at the most
constexpr int GA_ROW = 16;                      // doubles of a partial row
constexpr int GA_OBS_SUMS = 12;                 // of an observation's row in use: Q = sum g P^T (9), sum g (3)
constexpr int GA_MAX_VIEWS = 65535;             // grid.y

__host__ __device__ inline int slots_of(int64_t npix) {
  const int64_t chunks = (npix + GA_CHUNK - 1) / GA_CHUNK;
  return (int)(chunks < GA_SLOTS ? chunks : GA_SLOTS);
}

// vtab: int64 [N][3] = H, W, first element of the view in log_depth / d_log_depth, then the N + 1 starts of the observation lists.
// otab: int64 [2 E][4] = pointmap pointer, weight pointer, H, W of observation o = 2 e + side.  olist: the observations by view.
__global__ __launch_bounds__(GA_NT) void galign_main_kernel(const float* __restrict__ poses, const float* __restrict__ focals,
                                                            const float* __restrict__ pp, const float* __restrict__ log_depth,
                                                            const float* __restrict__ pw, const float* __restrict__ adapt,
                                                            const int64_t* __restrict__ vtab, int N, const int64_t* __restrict__ otab,
                                                            const int32_t* __restrict__ olist, double k0, double k1, int l2,
                                                            float* __restrict__ d_log_depth, double* __restrict__ vpart,
                                                            double* __restrict__ opart) {
  __shared__ double red[GA_NT / 64][GA_ROW];
  __shared__ double outb[GA_ROW];
  const int v = blockIdx.y, slot = blockIdx.x, tid = threadIdx.x;
  const int64_t W = vtab[3 * v + 1], npix = vtab[3 * v] * W, off = vtab[3 * v + 2];
  const int64_t chunks = (npix + GA_CHUNK - 1) / GA_CHUNK;
  const int S = slots_of(npix);
  if (slot >= S) return;  // the whole workgroup
  const int64_t* starts = vtab + 3 * (int64_t)N;
  const int64_t o0 = starts[v], o1 = starts[v + 1];
  double R[9], t[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)poses[12 * (int64_t)v + 4 * r + c];
    t[r] = (double)poses[12 * (int64_t)v + 4 * r + 3];
  }
  const double f = (double)focals[v], cx = (double)pp[2 * v], cy = (double)pp[2 * v + 1];
  double vacc[GA_ROW];
#pragma unroll
  for (int j = 0; j < GA_ROW; ++j) vacc[j] = 0.0;
  bool first = true;
  for (int64_t ch = slot; ch < chunks; ch += S) {
    double q[GA_PPT][3], X[GA_PPT][3], G[GA_PPT][3];
    int64_t pix[GA_PPT];
    bool live[GA_PPT];
#pragma unroll
    for (int k = 0; k < GA_PPT; ++k) {
      const int64_t p = ch * GA_CHUNK + (int64_t)k * GA_NT + tid;
      pix[k] = p;
      live[k] = p < npix;
#pragma unroll
      for (int c = 0; c < 3; ++c) q[k][c] = X[k][c] = G[k][c] = 0.0;
      if (live[k]) {
        const double d = exp((double)log_depth[off + p]);
        const double x = (double)(p % W), y = (double)(p / W);
        q[k][0] = (d * (x - cx)) / f;
        q[k][1] = (d * (y - cy)) / f;
        q[k][2] = d;
#pragma unroll
        for (int r = 0; r < 3; ++r) X[k][r] = ((R[3 * r] * q[k][0] + R[3 * r + 1] * q[k][1]) + R[3 * r + 2] * q[k][2]) + t[r];
      }
    }
    for (int64_t oi = o0; oi < o1; ++oi) {
      const int o = __builtin_amdgcn_readfirstlane(olist[oi]);
      const int e = o >> 1;
      const float* __restrict__ P = (const float*)otab[4 * (int64_t)o];
      const float* __restrict__ wmap = (const float*)otab[4 * (int64_t)o + 1];
      const double kk = (o & 1) ? k1 : k0;
      double Sm[9], m[3], a[3];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Sm[3 * r + c] = (double)pw[12 * (int64_t)e + 4 * r + c];
        m[r] = (double)pw[12 * (int64_t)e + 4 * r + 3];
        a[r] = (double)adapt[3 * (int64_t)e + r];
      }
      double oacc[GA_OBS_SUMS];
#pragma unroll
      for (int j = 0; j < GA_OBS_SUMS; ++j) oacc[j] = 0.0;
#pragma unroll
      for (int k = 0; k < GA_PPT; ++k) {
        if (!live[k]) continue;
        const double wt = (double)wmap[pix[k]];
        if (wt == 0.0) continue;  // a weight of exactly 0 contributes exactly nothing (a NaN weight goes on)
        const float* pt = P + 3 * pix[k];
        const double Pv[3] = {(double)pt[0], (double)pt[1], (double)pt[2]};
        const double b[3] = {a[0] * Pv[0], a[1] * Pv[1], a[2] * Pv[2]};
        double r[3], g[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] = X[k][i] - (((Sm[3 * i] * b[0] + Sm[3 * i + 1] * b[1]) + Sm[3 * i + 2] * b[2]) + m[i]);
        const double rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        double cost, s;
        if (l2) {
          cost = wt * rr;
          s = 2.0 * (kk * wt);
        } else {
          const double n = sqrt(rr);
          cost = wt * n;
          s = n == 0.0 ? 0.0 : (kk * wt) / n;  // torch's gradient of the norm at 0; a NaN norm stays NaN
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) g[i] = s * r[i];
        vacc[15] += kk * cost;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          G[k][i] += g[i];
#pragma unroll
          for (int c = 0; c < 3; ++c) oacc[3 * i + c] += g[i] * Pv[c];
          oacc[9 + i] += g[i];
        }
      }
      block_sum<GA_OBS_SUMS, GA_NT, GA_ROW>(oacc, red, outb);
      if (tid < GA_OBS_SUMS) {  // the word's one owner: reads back only what it wrote itself
        double* dst = opart + ((int64_t)o * GA_SLOTS + slot) * GA_ROW + tid;
        *dst = first ? outb[tid] : *dst + outb[tid];
      }
    }
#pragma unroll
    for (int k = 0; k < GA_PPT; ++k) {
      if (!live[k]) continue;
      double rq[3], u[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) rq[r] = (R[3 * r] * q[k][0] + R[3 * r + 1] * q[k][1]) + R[3 * r + 2] * q[k][2];
      d_log_depth[off + pix[k]] = (float)((G[k][0] * rq[0] + G[k][1] * rq[1]) + G[k][2] * rq[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) vacc[3 * i + c] += G[k][i] * q[k][c];
        vacc[9 + i] += G[k][i];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) u[c] = (R[c] * G[k][0] + R[3 + c] * G[k][1]) + R[6 + c] * G[k][2];
      vacc[12] += -((u[0] * q[k][0] + u[1] * q[k][1]) / f);
      const double df = q[k][2] / f;
      vacc[13] += -(df * u[0]);
      vacc[14] += -(df * u[1]);
    }
    first = false;
  }
  block_sum<GA_ROW, GA_NT, GA_ROW>(vacc, red, vpart + ((int64_t)v * GA_SLOTS + slot) * GA_ROW);
}

// one thread per output word: rows of a view, or of the two observations of an edge, in slot order from +0.0
__global__ __launch_bounds__(GA_NT) void galign_finish_kernel(const int64_t* __restrict__ vtab, int N, const int32_t* __restrict__ edges, int E,
                                                              const float* __restrict__ pw, const float* __restrict__ adapt,
                                                              const double* __restrict__ vpart, const double* __restrict__ opart,
                                                              float* __restrict__ d_poses, float* __restrict__ d_focals,
                                                              float* __restrict__ d_pp, float* __restrict__ d_pw, float* __restrict__ d_adapt,
                                                              double* __restrict__ lossv) {
  const int64_t idx = (int64_t)blockIdx.x * GA_NT + threadIdx.x;
  const int64_t nv = (int64_t)N * GA_ROW;
  if (idx < nv) {
    const int v = (int)(idx / GA_ROW), j = (int)(idx % GA_ROW);
    const int S = slots_of(vtab[3 * v] * vtab[3 * v + 1]);
    double s = 0.0;
    for (int sl = 0; sl < S; ++sl) s += vpart[((int64_t)v * GA_SLOTS + sl) * GA_ROW + j];
    if (j < 9) d_poses[12 * (int64_t)v + 4 * (j / 3) + j % 3] = (float)s;
    else if (j < 12) d_poses[12 * (int64_t)v + 4 * (j - 9) + 3] = (float)s;
    else if (j == 12) d_focals[v] = (float)s;
    else if (j < 15) d_pp[2 * (int64_t)v + (j - 13)] = (float)s;
    else lossv[v] = s;
    return;
  }
  const int64_t k = idx - nv;
  if (k >= (int64_t)E * GA_ROW) return;
  const int e = (int)(k / GA_ROW), j = (int)(k % GA_ROW);
  if (j == 15) return;
  auto word = [&](int k) {  // word k of the edge's rows: side 0's slots, then side 1's
    double s = 0.0;
    for (int side = 0; side < 2; ++side) {
      const int v = edges[2 * (int64_t)e + side];
      const int S = slots_of(vtab[3 * v] * vtab[3 * v + 1]);
      const int64_t o = 2 * (int64_t)e + side;
      for (int sl = 0; sl < S; ++sl) s += opart[(o * GA_SLOTS + sl) * GA_ROW + k];
    }
    return s;
  };
  if (j < 9) {  // dL/dS_ic = -Q_ic a_c
    d_pw[12 * (int64_t)e + 4 * (j / 3) + j % 3] = (float)(-(word(j) * (double)adapt[3 * (int64_t)e + j % 3]));
  } else if (j < 12) {  // dL/dm_i = -sum g_i
    d_pw[12 * (int64_t)e + 4 * (j - 9) + 3] = (float)(-word(j));
  } else {  // dL/da_c = -sum_i S_ic Q_ic
    const int c = j - 12;
    const float* Sm = pw + 12 * (int64_t)e;
    d_adapt[3 * (int64_t)e + c] = (float)(-(((double)Sm[c] * word(c) + (double)Sm[4 + c] * word(3 + c)) + (double)Sm[8 + c] * word(6 + c)));
  }
}

// the loss: thread t adds the views t, t + GA_NT, .. in ascending order, then one block_sum
__global__ __launch_bounds__(GA_NT) void galign_loss_kernel(const double* __restrict__ lossv, int N, double* __restrict__ loss) {
  __shared__ double red[GA_NT / 64][1];
  double s[1] = {0.0};
  for (int v = threadIdx.x; v < N; v += GA_NT) s[0] += lossv[v];
  block_sum<1, GA_NT, 1>(s, red, loss);
}

bool aligned(const void* p, size_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

size_t galign_ws_bytes(int N, int E) {
  return align256((size_t)N * GA_SLOTS * GA_ROW * sizeof(double)) + align256((size_t)2 * E * GA_SLOTS * GA_ROW * sizeof(double)) +
         align256((size_t)N * sizeof(double));
}

}  // namespace

extern "C" size_t f3r_galign_workspace_bytes(int n_views, int n_edges) {
  if (n_views < 2 || n_views > GA_MAX_VIEWS || n_edges < 1 || n_edges > (1 << 29)) return 0;
  return galign_ws_bytes(n_views, n_edges);
}

extern "C" int f3r_galign_loss_grad(const float* poses, const float* focals, const float* pp, const float* log_depth, const float* pw_poses,
                                    const float* adaptors, const int64_t* view_table, const int64_t* view_table_host, int n_views,
                                    const int32_t* edges, const int32_t* edges_host, int n_edges, const int64_t* obs_table,
                                    const int64_t* obs_table_host, const int32_t* obs_list, const int32_t* obs_list_host, int dist, double* loss,
                                    float* d_log_depth, float* d_poses, float* d_focals, float* d_pp, float* d_pw_poses, float* d_adaptors,
                                    void* workspace, size_t workspace_bytes, f3r_stream_t stream) {
  const int N = n_views, E = n_edges;
  F3R_REQUIRE(N >= 2 && N <= GA_MAX_VIEWS, "f3r_galign_loss_grad: n_views = %d; need 2 .. %d views", N, GA_MAX_VIEWS);
  F3R_REQUIRE(E >= 1 && E <= (1 << 29), "f3r_galign_loss_grad: n_edges = %d; need 1 .. 2^29 edges", E);
  F3R_REQUIRE(poses && focals && pp && log_depth && pw_poses && adaptors && view_table && view_table_host && edges && edges_host && obs_table &&
                  obs_table_host && obs_list && obs_list_host && loss && d_log_depth && d_poses && d_focals && d_pp && d_pw_poses && d_adaptors &&
                  workspace,
              "f3r_galign_loss_grad: null pointer");
  F3R_REQUIRE(dist == F3R_GALIGN_L1 || dist == F3R_GALIGN_L2, "f3r_galign_loss_grad: dist = %d (F3R_GALIGN_L1 or F3R_GALIGN_L2)", dist);
  int64_t run = 0;
  for (int v = 0; v < N; ++v) {
    const int64_t H = view_table_host[3 * v], W = view_table_host[3 * v + 1];
    F3R_REQUIRE(H >= 1 && W >= 1 && H <= (int64_t)0x7fffffff && W <= (int64_t)0x7fffffff && H * W <= (int64_t)0x7fffffff,
                "f3r_galign_loss_grad: view %d is %lld x %lld; need H, W >= 1 and H W <= 2^31 - 1", v, (long long)H, (long long)W);
    F3R_REQUIRE(view_table_host[3 * v + 2] == run, "f3r_galign_loss_grad: the offset of view %d is %lld, the running sum of the shapes is %lld", v,
                (long long)view_table_host[3 * v + 2], (long long)run);
    run += H * W;
  }
  double area[2] = {0.0, 0.0};
  for (int e = 0; e < E; ++e) {
    const int i = edges_host[2 * (int64_t)e], j = edges_host[2 * (int64_t)e + 1];
    F3R_REQUIRE(i >= 0 && i < N && j >= 0 && j < N, "f3r_galign_loss_grad: edge %d = (%d, %d) lies outside the %d views", e, i, j, N);
    F3R_REQUIRE(i != j, "f3r_galign_loss_grad: edge %d joins view %d with itself", e, i);
    for (int side = 0; side < 2; ++side) {
      const int v = side ? j : i;
      const int64_t* row = obs_table_host + 4 * (2 * (int64_t)e + side);
      F3R_REQUIRE(row[0] != 0 && row[1] != 0, "f3r_galign_loss_grad: null pointmap or weight map of edge %d, side %d", e, side);
      F3R_REQUIRE((row[0] & 3) == 0 && (row[1] & 3) == 0, "f3r_galign_loss_grad: misaligned pointmap or weight map of edge %d, side %d", e, side);
      F3R_REQUIRE(row[2] == view_table_host[3 * v] && row[3] == view_table_host[3 * v + 1],
                  "f3r_galign_loss_grad: the observation of edge %d, side %d is %lld x %lld, its view %d is %lld x %lld", e, side, (long long)row[2],
                  (long long)row[3], v, (long long)view_table_host[3 * v], (long long)view_table_host[3 * v + 1]);
      area[side] += (double)(row[2] * row[3]);
    }
  }
  const int64_t* starts_host = view_table_host + 3 * (int64_t)N;
  F3R_REQUIRE(starts_host[0] == 0 && starts_host[N] == 2 * (int64_t)E,
              "f3r_galign_loss_grad: the observation lists must start at 0 and end at 2 n_edges = %lld", (long long)(2 * (int64_t)E));
  for (int v = 0; v < N; ++v) {
    const int64_t a = starts_host[v], b = starts_host[v + 1];
    F3R_REQUIRE(a <= b && b <= 2 * (int64_t)E, "f3r_galign_loss_grad: the observation list of view %d is [%lld, %lld) of %lld", v, (long long)a,
                (long long)b, (long long)(2 * (int64_t)E));
    for (int64_t k = a; k < b; ++k) {
      const int64_t o = obs_list_host[k];
      F3R_REQUIRE(o >= 0 && o < 2 * (int64_t)E && edges_host[o] == v, "f3r_galign_loss_grad: observation %lld in the list of view %d is not one of its own",
                  (long long)o, v);  // edges_host[2 e + side] is the view of observation 2 e + side
      F3R_REQUIRE(k == a || obs_list_host[k - 1] < o, "f3r_galign_loss_grad: the observations of view %d must ascend", v);
    }
  }  // 2 E entries, each its view's own, ascending within a view: every observation is listed once
  F3R_REQUIRE(workspace_bytes >= galign_ws_bytes(N, E) && aligned(workspace, 256), "f3r_galign_loss_grad: workspace too small / misaligned");
  F3R_REQUIRE(aligned(poses, 4) && aligned(focals, 4) && aligned(pp, 4) && aligned(log_depth, 4) && aligned(pw_poses, 4) && aligned(adaptors, 4) &&
                  aligned(view_table, 8) && aligned(edges, 4) && aligned(obs_table, 8) && aligned(obs_list, 4) && aligned(loss, 8) &&
                  aligned(d_log_depth, 4) && aligned(d_poses, 4) && aligned(d_focals, 4) && aligned(d_pp, 4) && aligned(d_pw_poses, 4) &&
                  aligned(d_adaptors, 4),
              "f3r_galign_loss_grad: misaligned buffer");
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)workspace;
  double* vpart = (double*)base;
  double* opart = (double*)(base + align256((size_t)N * GA_SLOTS * GA_ROW * sizeof(double)));
  double* lossv = (double*)((char*)opart + align256((size_t)2 * E * GA_SLOTS * GA_ROW * sizeof(double)));
  hipLaunchKernelGGL(galign_main_kernel, dim3(GA_SLOTS, N), dim3(GA_NT), 0, s, poses, focals, pp, log_depth, pw_poses, adaptors, view_table, N,
                     obs_table, obs_list, 1.0 / area[0], 1.0 / area[1], dist == F3R_GALIGN_L2 ? 1 : 0, d_log_depth, vpart, opart);
  const int64_t words = ((int64_t)N + E) * GA_ROW;
  hipLaunchKernelGGL(galign_finish_kernel, dim3(blocks_of(words, GA_NT)), dim3(GA_NT), 0, s, view_table, N, edges, E, pw_poses, adaptors, (const double*)vpart,
                     (const double*)opart, d_poses, d_focals, d_pp, d_pw_poses, d_adaptors, lossv);
  hipLaunchKernelGGL(galign_loss_kernel, dim3(1), dim3(GA_NT), 0, s, (const double*)lossv, N, loss);
  return f3r_check_launch("f3r_galign_loss_grad");
}
