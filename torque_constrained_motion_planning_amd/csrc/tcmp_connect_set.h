// tcmp_connect_set.h -- goal-set connection (tcmp_connect_goal_set, tcmp_plan_connect_goal_set):
// the stage of tcmp_connect.h with one change, each node is tried toward the goal of a given set
// G_0 .. G_{n-1} (n <= 256) that is nearest to it.  A grasp pose has a family of goal
// configurations (joint 7 is free, up to 8 IK branches per value; tcmp_goal_search lists them);
// the rounds and tcmp_plan_connect aim at one of them.  Opt-in, deterministic, no RNG.
//
// include/tcmp.h and DESIGN §3 state the definition; tests/connect_set_ref.py is the oracle.  The
// selection (k_cn_hist, k_cn_compact, the two rocPRIM sorts), launch_edges and the host's waits
// are cn_run's own; what differs hangs on its `sg` (CsStage below):
//   k_cs_keys     one node per thread: s_ij = sum_k w_k (G_jk - c_ik)^2 over the goals, scanned
//                 j ascending with a running (s_min, j_min) under a strict <, so the lowest j of
//                 equal sums stays and a NaN sum never wins; key_i = g_i + sqrt(s_min), stored
//                 and reduced as k_cn_keys does.  The goals (at most 14,336 B) and the weights
//                 are staged once per block in LDS: every lane reads the same address, which the
//                 LDS broadcasts, and the loop needs no registers for a goal row.  near[j] counts
//                 the eligible nodes whose goal is j: a per-block LDS histogram, then integer
//                 global atomics
//   k_cs_targets  per pass, for ranks [r0, r0 + n): the node's goal j* recomputed by the same
//                 device function (cs_nearest: the same operations in the same order, so the same
//                 bits -- no byte per node is kept, the tree-proportional memory stays the one
//                 8-byte key), its row into the pass's `to` buffer, j* into the ranks' index list
//   k_cs_pick     k_cn_pick with the candidate's own goal row in the tolerance test and as the
//                 appended node's extend target, per-goal tested / valid counts through LDS
//                 integer atomics, and the winner's goal index beside the pick record
// Only integer atomics; no workgroup waits on another one.
#pragma once

namespace {

constexpr int kCsMaxGoals = 256;

// j*(c): the lowest j attaining min_j s_j, and that minimum in s_min (INFINITY: every sum is
// NaN or infinite, j* = 0).  G: n rows of 7.
__device__ __forceinline__ int cs_nearest(const double c[7], const double* G, const double* w,
                                          int n, double& s_min) {
#pragma clang fp contract(off)
  double sm = INFINITY;
  int jm = 0;
  for (int j = 0; j < n; ++j) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const double d = G[7 * j + k] - c[k];
      s += w[k] * (d * d);
    }
    if (s < sm) {
      sm = s;
      jm = j;
    }
  }
  s_min = sm;
  return jm;
}

// ------------------------------------------------------------------------------------------
// k_cs_keys.  st, bound: as k_cn_keys.  near: n counts, zeroed before.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cs_keys(const PlanParams* __restrict__ Pd,
                                                 const double* __restrict__ rows, long long T,
                                                 const DevState* st, double bound,
                                                 const double* __restrict__ goals, int n,
                                                 unsigned long long* __restrict__ key, CnState* cs,
                                                 unsigned long long* near) {
#pragma clang fp contract(off)
  __shared__ double sG[kCsMaxGoals * 7];
  __shared__ double sw[7];
  __shared__ unsigned sh[kCsMaxGoals];
  for (int i = threadIdx.x; i < 7 * n; i += 256) sG[i] = goals[i];
  if (threadIdx.x < 7) sw[threadIdx.x] = Pd->w[threadIdx.x];
  sh[threadIdx.x] = 0;
  __syncthreads();
  const long long g = st ? st->goal_node : -1;
  const double B = st ? (g >= 0 ? rows[8 * g + 7] : INFINITY) : bound;
  unsigned long long cnt = 0, mn = kCnNone;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < T; i += stride) {
    double c[7], sm;
    load7(rows + 8 * i, c);
    const int jm = cs_nearest(c, sG, sw, n, sm);
    const double kx = rows[8 * i + 7] + sqrt(sm);
    const bool ok = kx < B;  // (a NaN key fails)
    const unsigned long long b = ok ? (unsigned long long)__double_as_longlong(kx) : kCnNone;
    key[i] = b;
    if (ok) {
      ++cnt;
      mn = b < mn ? b : mn;
      atomicAdd(&sh[jm], 1u);
    }
  }
  cnt = wave_sum_u64(cnt);
  mn = wave_min_u64(mn);
  if (lane_id() == 0 && cnt) {
    atomicAdd(&cs->n_eligible, cnt);
    atomicMin(&cs->key_min, mn);
  }
  __syncthreads();
  if ((int)threadIdx.x < n && sh[threadIdx.x])
    atomicAdd(&near[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cs->goal_before = g;
    cs->bound = B;
    cs->cost_before = g >= 0 ? B : 0.0;
  }
}

// ------------------------------------------------------------------------------------------
// k_cs_targets: edge e of the pass is rank r0 + e; to[e] = G_{j*}, gidx[r0 + e] = j*
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cs_targets(const PlanParams* __restrict__ Pd,
                                                    const double* __restrict__ rows,
                                                    const int* __restrict__ ids,
                                                    const double* __restrict__ goals, int ng,
                                                    int r0, int n, double* __restrict__ to,
                                                    int* __restrict__ gidx) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double c[7], w[7], sm;
  load7(rows + 8 * (long long)ids[r0 + e], c);
#pragma unroll
  for (int k = 0; k < 7; ++k) w[k] = Pd->w[k];
  const int j = cs_nearest(c, goals, w, ng, sm);
#pragma unroll
  for (int k = 0; k < 7; ++k) to[8 * (size_t)e + k] = goals[7 * j + k];
  to[8 * (size_t)e + 7] = 0.0;
  gidx[r0 + e] = j;
}

// ------------------------------------------------------------------------------------------
// k_cs_pick: one block; k_cn_pick's pass outcome with G_{gidx[rank]} in G's place.  tab: the
// per-goal counts (near, tested, valid: ng each), then the winner's goal index.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_cs_pick(const PlanParams* __restrict__ Pd,
                                                  const double* __restrict__ rows,
                                                  const int* __restrict__ ids,
                                                  const int* __restrict__ nsafe,
                                                  const int* __restrict__ nsteps,
                                                  const double* __restrict__ last,
                                                  const double* __restrict__ goals, int ng,
                                                  const int* __restrict__ gidx, int r0, int n,
                                                  const CnState* __restrict__ cs, DevState* st,
                                                  Tree tr, long long max_nodes, CnPick* out,
                                                  long long* tab) {
#pragma clang fp contract(off)
  __shared__ double wm[16];
  __shared__ int wk[16];
  __shared__ unsigned long long s_valid;
  __shared__ unsigned s_tested[kCsMaxGoals], s_ok[kCsMaxGoals];
  const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  double w[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) w[k] = Pd->w[k];
  const double tol = Pd->goal_tol, B = cs->bound;
  if (tid == 0) s_valid = 0;
  if (tid < kCsMaxGoals) s_tested[tid] = s_ok[tid] = 0;
  __syncthreads();
  double bc = INFINITY;
  int be = INT_MAX;
  unsigned long long nv = 0;
  for (int e = tid; e < n; e += 1024) {
    const int j = gidx[r0 + e];
    atomicAdd(&s_tested[j], 1u);
    if (nsafe[r0 + e] <= 0) continue;
    double lq[7], pc[7], G[7];
    load7(last + 8 * (size_t)e, lq);
    load7u(goals + 7 * j, G);
    if (!(distance(lq, G, w) < tol)) continue;
    ++nv;
    atomicAdd(&s_ok[j], 1u);
    const long long i = ids[r0 + e];
    load7(rows + 8 * i, pc);
    const double c = rows[8 * i + 7] + distance(pc, lq, w);
    if (c < B && c < bc) {  // (e ascends: the first of equal costs stays)
      bc = c;
      be = e;
    }
  }
  nv = wave_sum_u64(nv);
  const double mn = wave_min(bc);
  const int wi = wave_min_int(bc == mn ? be : INT_MAX);
  if (lane == 0) {
    wm[wave] = mn;
    wk[wave] = wi;
    if (nv) atomicAdd(&s_valid, nv);
  }
  __syncthreads();
  if (tid < ng) {  // (the passes follow one another on the stream: plain sums)
    tab[ng + tid] += s_tested[tid];
    tab[2 * ng + tid] += s_ok[tid];
  }
  if (tid != 0) return;
  double best = INFINITY;
  int bk = INT_MAX;
  for (int q = 0; q < 16; ++q)
    if (wk[q] != INT_MAX && (wm[q] < best || (wm[q] == best && wk[q] < bk))) {
      best = wm[q];
      bk = wk[q];
    }
  CnPick p{};
  p.n_valid = s_valid;
  p.rank = p.parent = -1;
  p.node = -1;
  if (bk != INT_MAX) {
    const int j = gidx[r0 + bk];
    p.found = 1;
    p.rank = r0 + bk;
    p.parent = ids[r0 + bk];
    p.nsteps = nsteps[r0 + bk];
    p.nsafe = nsafe[r0 + bk];
    p.c = best;
    double lq[7];
    load7(last + 8 * (size_t)bk, lq);
#pragma unroll
    for (int k = 0; k < 7; ++k) p.last[k] = lq[k];
    if (tr.cfg) {
      const long long T = st->n_nodes;
      if (T >= max_nodes) {
        p.full = 1;
      } else {
        double G[7];
        load7u(goals + 7 * j, G);
        double* dst = tr.cfg + 8 * T;
        store7(dst, lq);
        dst[7] = best;
        tr.parent[T] = p.parent;
        store7(tr.tgt + 8 * T, G);
        tr.tgt[8 * T + 7] = 0.0;
        tr.meta[T] = make_int2(p.nsteps, p.nsafe);
        st->n_nodes = T + 1;
        st->goal_node = T;
        p.node = T;
      }
    }
    tab[3 * ng] = j;
  }
  *out = p;
}

// cn_run's hooks for a goal set: n goals on the device (h->cset_goals), the counts and the
// ranks' goal indices in h->cset_tab and h->cset_gidx, and their host copies after the last wait
struct CsStage {
  int n;
  int32_t* gidx_out;            // the ranks' goal indices (null: not wanted)
  std::vector<long long> tab;   // near, tested, valid (n each), the winner's goal index

  CsStage(int n_goals, int32_t* gout) : n(n_goals), gidx_out(gout), tab(3 * (size_t)n_goals + 1, 0) {
    tab.back() = -1;
  }
  void keys(tcmp_handle* h, unsigned grid, const PlanParams* dP, const double* rows, long long T,
            const DevState* st, double bound, CnState* cs) {
    hipLaunchKernelGGL(k_cs_keys, dim3(grid), dim3(256), 0, h->stream, dP, rows, T, st, bound,
                       h->cset_goals.p, n, h->cn_key.p, cs,
                       reinterpret_cast<unsigned long long*>(h->cset_tab.p));
  }
  int targets(tcmp_handle* h, const PlanParams*, size_t, size_t m) {
    if (int rc = h->cset_gidx.ensure(m)) return rc;
    HIPCHK(hipMemsetAsync(h->cset_gidx.p, 0xFF, m * sizeof(int), h->stream));  // -1: not tested
    return 0;
  }
  void pass_targets(tcmp_handle* h, const PlanParams* dP, const double* rows, const int* ids,
                    int r0, int cnt) {
    hipLaunchKernelGGL(k_cs_targets, dim3(grid_for(cnt, 256)), dim3(256), 0, h->stream, dP, rows,
                       ids, h->cset_goals.p, n, r0, cnt, h->cn_to.p, h->cset_gidx.p);
  }
  void pick(tcmp_handle* h, const PlanParams* dP, const double* rows, const int* ids, int r0,
            int cnt, const CnState* cs, DevState* st, Tree tr, long long max_nodes, CnPick* dpick) {
    hipLaunchKernelGGL(k_cs_pick, dim3(1), dim3(1024), 0, h->stream, dP, rows, ids, h->cn_nsafe.p,
                       h->cn_nsteps.p, h->cn_last.p, h->cset_goals.p, n, h->cset_gidx.p, r0, cnt,
                       cs, st, tr, max_nodes, dpick, h->cset_tab.p);
  }
  int finish(tcmp_handle* h, size_t m) {
    if (int rc = download(h, tab.data(), h->cset_tab.p, tab.size())) return rc;
    return gidx_out ? download(h, gidx_out, h->cset_gidx.p, m) : 0;
  }
};

// the goals' checks (nothing is queued before they pass)
int cs_check(const double* goals, int32_t n_goals) {
  if (!goals || n_goals < 1 || n_goals > kCsMaxGoals) return fail(-1, "n_goals outside [1, 256]");
  for (int i = 0; i < 7 * n_goals; ++i)
    if (!std::isfinite(goals[i])) return fail(-1, "a goal value is not finite");
  return 0;
}

// the goals' upload, and the counts zeroed (the winner's goal index: -1)
int cs_goals(tcmp_handle* h, const double* goals, int32_t n_goals) {
  if (int rc = h->cset_tab.ensure(3 * (size_t)n_goals + 1)) {
    (void)hipStreamSynchronize(h->stream);  // (the caller's arrays may be queued already)
    return rc;
  }
  if (int rc = upload(h, h->cset_goals, goals, 7 * (size_t)n_goals)) return rc;
  long long* t = h->cset_tab.p;
  HIPCHK(hipMemsetAsync(t, 0, 3 * (size_t)n_goals * sizeof(long long), h->stream));
  HIPCHK(hipMemsetAsync(t + 3 * n_goals, 0xFF, sizeof(long long), h->stream));
  return 0;
}

void cs_report(const CsStage& sg, int64_t* per_goal, tcmp_connect_set_result* res) {
  res->n_goals = sg.n;
  res->goal_index = (int32_t)sg.tab.back();
  if (per_goal) memcpy(per_goal, sg.tab.data(), 3 * (size_t)sg.n * sizeof(int64_t));
}

}  // namespace

extern "C" {

int tcmp_connect_goal_set(tcmp_handle* h, const double* nodes, const double* cost, int64_t n,
                          const double* goals, int32_t n_goals, double bound,
                          const double* resolutions, const double* weights, double goal_tolerance,
                          int32_t torque_mode, double payload_mass, const tcmp_connect_cfg* cfg,
                          int32_t* ids_out, double* keys_out, int32_t* goal_out,
                          int32_t* nsafe_out, int32_t* nsteps_out, int64_t cap_out,
                          double* node_out, int64_t* per_goal, tcmp_connect_set_result* res) {
  TCMP_ENTER(h);
  if (int rc = cs_check(goals, n_goals)) return rc;
  int K, passes;
  PlanParams P;
  std::vector<double> tmp;
  if (int rc = cn_stage(h, nodes, cost, n, goals, bound, resolutions, weights, goal_tolerance,
                        torque_mode, payload_mass, cap_out, cfg, res, sizeof(*res), &K, &passes, P,
                        tmp))
    return rc;
  if (int rc = cs_goals(h, goals, n_goals)) return rc;
  const CnOut o{ids_out, keys_out, nsafe_out, nsteps_out, cap_out, node_out, goal_out};
  CsStage sg(n_goals, goal_out);
  const int rc = cn_run(h, h->dPx, h->cn_rows.p, n, nullptr, Tree{}, 0, bound, K, passes, &o,
                        &res->r, sg);
  res->n_goals = n_goals;
  res->goal_index = -1;
  if (rc) return rc;
  cs_report(sg, per_goal, res);
  return 0;
}

int tcmp_plan_connect_goal_set(tcmp_handle* h, const double* goals, int32_t n_goals,
                               const tcmp_connect_cfg* cfg, int64_t* per_goal,
                               tcmp_connect_set_result* res) {
  TCMP_ENTER(h);
  if (!res) return fail(-1, "null result");
  if (!h->plan_open) return fail(-1, "no open plan");
  int K, passes;
  if (int rc = cn_cfg(cfg, &K, &passes)) return rc;
  if (int rc = cs_check(goals, n_goals)) return rc;
  memset(res, 0, sizeof(*res));
  res->goal_index = -1;
  long long T = 0;
  HIPCHK(hipMemcpyAsync(&T, &h->st->n_nodes, sizeof(T), hipMemcpyDeviceToHost, h->stream));
  if (int rc_s = sync_stream(h)) return rc_s;
  if (T < 1 || T > INT_MAX) return fail(-1, "no tree to connect");
  if (int rc = cs_goals(h, goals, n_goals)) return rc;
  CsStage sg(n_goals, nullptr);
  if (int rc = cn_run(h, h->dP, h->cfg.p, T, h->st, Tree{h->cfg.p, h->parent.p, h->tgt.p, h->meta.p},
                      h->P.max_nodes, INFINITY, K, passes, nullptr, &res->r, sg))
    return rc;
  cs_report(sg, per_goal, res);
  if (res->r.status == TCMP_CONNECT_OK) {
    // (as tcmp_plan_connect: the host's bound on the tree size, the stored list, the rows)
    ++h->extra_nodes;
    h->sc_live = false;
    h->fin_status = -1;
  }
  return 0;
}

}  // extern "C"
