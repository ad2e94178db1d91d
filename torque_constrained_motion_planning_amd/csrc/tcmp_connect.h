// tcmp_connect.h -- best-parent goal connection over the whole tree (tcmp_connect_nodes,
// tcmp_plan_connect): an opt-in stage between the rounds and the shortcut or finish.  The rounds
// try the goal only from the node nearest to it, on one goal-biased lane per round, and never
// again once a goal node exists; the shortcut straightens a path that already exists but cannot
// find a goal or change to another branch.  Here every node i of the tree is ranked by
// key_i = cost_i + distance(c_i, G), the cost of a goal reached straight from it, the best
// K * passes of those that could beat the current goal cost go through the tree edges' own check
// (launch_edges: safe_path_force_aware(extend(c_i, G)), static torque test), and the cheapest one
// that reaches the goal becomes the goal node's parent.  Deterministic, no RNG.
//
// include/tcmp.h and DESIGN §3 state the definition; tests/connect_ref.py is the oracle.  Stages:
//   k_cn_keys      one node per thread: the key as its 64-bit integer image (non-negative doubles
//                  order as unsigned integers; all ones: not eligible), the eligible count and the
//                  smallest key by wave reductions and integer atomics
//   k_cn_hist      device-wide radix select of the M-th smallest composite (key bits, index), top
//                  down by 8-bit digits -- eight of the key, four of the index; the composite is
//                  unique, so there are no ties.  A pass is one streaming launch: per-block LDS
//                  histograms of the rows that match the digits chosen so far, then integer
//                  global atomics; the next launch chooses the digit from the finished histogram
//   k_cn_compact   the composites at or below the threshold, M of them, in any order
//   rocPRIM        two stable radix sorts of the M rows (by index, then by key): (key, index) order
//   per pass       launch_edges from the tree rows of K ranks to rows of G, then the one-block
//                  k_cn_pick: validity, the new cost, the (cost, rank) minimum, the node write
// No workgroup waits on another one anywhere: every dependence is a kernel boundary.  Device
// memory proportional to the tree is the one 8-byte key per node.
// The goal-set stage (tcmp_connect_set.h) shares cn_run: the key, target and pick launches come
// from a stage object, CnSingle for the single goal.
#pragma once

namespace {

constexpr int kCnMaxCand = 65536;  // max_candidates
constexpr int kCnMaxPasses = 8;
constexpr int kCnDigits = 12;      // 8-bit digits of the composite: 8 of the key, 4 of the index
constexpr unsigned long long kCnNone = ~0ull;

// the selection's device state; zeroed (key_min: all ones) before k_cn_keys
struct CnState {
  unsigned long long n_eligible, key_min;
  long long goal_before;       // the goal node k_cn_keys saw (-1: none)
  double bound, cost_before;   // B; the goal node's cost (0 without one)
  unsigned cnt, pad;           // rows k_cn_compact has taken
  // after d digits: the chosen digits in place, and the rank wanted among the rows matching them
  unsigned long long pk[kCnDigits + 1], k[kCnDigits + 1];
  unsigned pi[kCnDigits + 1];
  unsigned hist[kCnDigits][256];
};

// one pass's outcome (k_cn_pick)
struct CnPick {
  int found, full;  // a winner; it could not be appended (the tree is at max_nodes)
  int rank, parent, nsteps, nsafe;
  long long node;   // the appended node (-1: none)
  unsigned long long n_valid;
  double c, last[7];
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long y = __shfl_xor(x, o);
    x = y < x ? y : x;
  }
  return x;
}

// ------------------------------------------------------------------------------------------
// k_cn_keys.  st: the open plan's state (B is the goal node's cost, read from its tree row), or
// null (B = bound).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cn_keys(const PlanParams* __restrict__ Pd,
                                                 const double* __restrict__ rows, long long T,
                                                 const DevState* st, double bound,
                                                 unsigned long long* __restrict__ key,
                                                 CnState* cs) {
#pragma clang fp contract(off)
  const long long g = st ? st->goal_node : -1;
  const double B = st ? (g >= 0 ? rows[8 * g + 7] : INFINITY) : bound;
  double G[7], w[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    G[k] = Pd->goal[k];
    w[k] = Pd->w[k];
  }
  unsigned long long cnt = 0, mn = kCnNone;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < T; i += stride) {
    double c[7];
    load7(rows + 8 * i, c);
    const double kx = rows[8 * i + 7] + distance(c, G, w);
    const bool ok = kx < B;  // (a NaN key fails)
    const unsigned long long b = ok ? (unsigned long long)__double_as_longlong(kx) : kCnNone;
    key[i] = b;
    if (ok) {
      ++cnt;
      mn = b < mn ? b : mn;
    }
  }
  cnt = wave_sum_u64(cnt);
  mn = wave_min_u64(mn);
  if (lane_id() == 0 && cnt) {
    atomicAdd(&cs->n_eligible, cnt);
    atomicMin(&cs->key_min, mn);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cs->goal_before = g;
    cs->bound = B;
    cs->cost_before = g >= 0 ? B : 0.0;
  }
}

// The digits chosen so far, for a block of 256 threads: from the state after d - 1 digits and
// the finished histogram of digit d - 1, the state after d digits (d = 0: nothing chosen, the
// rank wanted is k0).  Every block derives it for itself; block 0 also stores it for the next
// launch.
__device__ __forceinline__ void cn_choose(CnState* cs, int d, unsigned long long k0,
                                          unsigned long long& pk, unsigned& pi,
                                          unsigned long long& k) {
  __shared__ unsigned long long sc[256];
  __shared__ unsigned long long s_pk, s_k;
  __shared__ unsigned s_pi;
  const int tid = threadIdx.x;
  if (d == 0) {
    pk = 0;
    pi = 0;
    k = k0;
  } else {
    const unsigned long long v = cs->hist[d - 1][tid];
    sc[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const unsigned long long x = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += x;
      __syncthreads();
    }
    const unsigned long long kp = cs->k[d - 1], excl = sc[tid] - v;
    if (excl <= kp && kp < sc[tid]) {  // one thread: its digit holds the wanted rank
      const int e = d - 1;
      unsigned long long q = cs->pk[e];
      unsigned qi = cs->pi[e];
      if (e < 8) q |= (unsigned long long)tid << (56 - 8 * e);
      else qi |= (unsigned)tid << (24 - 8 * (e - 8));
      s_pk = q;
      s_pi = qi;
      s_k = kp - excl;
    }
    __syncthreads();
    pk = s_pk;
    pi = s_pi;
    k = s_k;
  }
  if (blockIdx.x == 0 && tid == 0) {
    cs->pk[d] = pk;
    cs->pi[d] = pi;
    cs->k[d] = k;
  }
}

// ------------------------------------------------------------------------------------------
// k_cn_hist: digit d's histogram over the eligible rows that match the d digits chosen so far
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cn_hist(const unsigned long long* __restrict__ key,
                                                 long long T, int d, unsigned long long k0,
                                                 CnState* cs) {
  __shared__ unsigned lh[256];
  unsigned long long pk, k;
  unsigned pi;
  lh[threadIdx.x] = 0;
  cn_choose(cs, d, k0, pk, pi, k);
  __syncthreads();
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < T; i += stride) {
    const unsigned long long b = key[i];
    if (b == kCnNone) continue;
    if (d < 8) {
      const int s = 56 - 8 * d;
      if (d == 0 || (b >> (s + 8)) == (pk >> (s + 8))) atomicAdd(&lh[(b >> s) & 255u], 1u);
    } else if (b == pk) {
      const int s = 24 - 8 * (d - 8);
      const unsigned x = (unsigned)i;
      if (d == 8 || (x >> (s + 8)) == (pi >> (s + 8))) atomicAdd(&lh[(x >> s) & 255u], 1u);
    }
  }
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&cs->hist[d][threadIdx.x], lh[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------
// k_cn_compact: the rows whose composite is at or below the threshold the twelve digits spell
// (all != 0: every eligible row, M = n_eligible), M of them, in the order the waves arrive --
// the sorts that follow fix the order
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cn_compact(const unsigned long long* __restrict__ key,
                                                    long long T, int all, unsigned M, CnState* cs,
                                                    unsigned long long* __restrict__ okey,
                                                    unsigned* __restrict__ oidx) {
  unsigned long long tk = kCnNone, k = 0;
  unsigned ti = ~0u;
  if (!all) cn_choose(cs, kCnDigits, 0, tk, ti, k);
  const int lane = lane_id();
  const long long stride = (long long)gridDim.x * 256;
  // (whole waves go round together: the ballot needs every lane of a wave that has one in range)
  for (long long i0 = (long long)blockIdx.x * 256; i0 < T; i0 += stride) {
    const long long i = i0 + threadIdx.x;
    const unsigned long long b = i < T ? key[i] : kCnNone;
    const bool take = b != kCnNone && (b < tk || (b == tk && (unsigned)i <= ti));
    const uint64_t m = __ballot(take);
    if (!m) continue;
    const int leader = __builtin_ctzll(m);
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(&cs->cnt, (unsigned)__popcll(m));
    base = __shfl(base, leader);
    if (take) {
      const unsigned pos = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
      if (pos < M) {
        okey[pos] = b;
        oidx[pos] = (unsigned)i;
      }
    }
  }
}

// n rows of G as EdgeJob::to reads them
__global__ __launch_bounds__(256) void k_cn_targets(const PlanParams* __restrict__ Pd, int n,
                                                    double* to) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
#pragma unroll
  for (int k = 0; k < 7; ++k) to[8 * (size_t)e + k] = Pd->goal[k];
  to[8 * (size_t)e + 7] = 0.0;
}

// ------------------------------------------------------------------------------------------
// k_cn_pick: one block.  The pass's n edges are ranks r0 .. r0 + n - 1 (ids, nsafe, nsteps are
// indexed by rank, last by edge).  A candidate is valid iff n_safe > 0 and its last point lies
// within goal_tol of G (k_ins_write's test of a goal lane); its cost is c = cost_i +
// distance(c_i, last); the winner is the valid one with c < B smallest by (c, rank): the DPP wave
// minimum on c, then on the rank among the lanes that hold it, then the waves' minima in turn.
// tr.cfg != null (the plan form): the winner is appended at n_nodes with k_ins_write's record and
// becomes the goal node -- unless the tree is full.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_cn_pick(const PlanParams* __restrict__ Pd,
                                                  const double* __restrict__ rows,
                                                  const int* __restrict__ ids,
                                                  const int* __restrict__ nsafe,
                                                  const int* __restrict__ nsteps,
                                                  const double* __restrict__ last, int r0, int n,
                                                  const CnState* __restrict__ cs, DevState* st,
                                                  Tree tr, long long max_nodes, CnPick* out) {
#pragma clang fp contract(off)
  __shared__ double wm[16];
  __shared__ int wk[16];
  __shared__ unsigned long long s_valid;
  const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  double G[7], w[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    G[k] = Pd->goal[k];
    w[k] = Pd->w[k];
  }
  const double tol = Pd->goal_tol, B = cs->bound;
  if (tid == 0) s_valid = 0;
  __syncthreads();
  double bc = INFINITY;
  int be = INT_MAX;
  unsigned long long nv = 0;
  for (int e = tid; e < n; e += 1024) {
    if (nsafe[r0 + e] <= 0) continue;
    double lq[7], pc[7];
    load7(last + 8 * (size_t)e, lq);
    if (!(distance(lq, G, w) < tol)) continue;
    ++nv;
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
  }
  *out = p;
}

int cn_cfg(const tcmp_connect_cfg* cfg, int* K, int* passes) {
  *K = cfg && cfg->max_candidates ? cfg->max_candidates : 1024;
  *passes = cfg && cfg->passes ? cfg->passes : 1;
  if (*K < 1 || *K > kCnMaxCand) return fail(-1, "max_candidates outside [1, 65536]");
  if (*passes < 1 || *passes > kCnMaxPasses) return fail(-1, "passes outside [1, 8]");
  return 0;
}

// what the stand-alone form hands back (null: not wanted)
struct CnOut {
  int32_t* ids;
  double* keys;
  int32_t* nsafe;
  int32_t* nsteps;
  int64_t cap;
  double* node;
  int32_t* gidx = nullptr;  // the goal-set stage's: the ranks' goal indices
};

// What the goal-set stage (tcmp_connect_set.h) does differently hangs on cn_run's `sg`: the key
// kernel, where the passes' targets come from, the pick kernel, and what else comes back.  This
// is the single goal's: the launches below are the stage's own, in the order it always had.
struct CnSingle {
  void keys(tcmp_handle* h, unsigned grid, const PlanParams* dP, const double* rows, long long T,
            const DevState* st, double bound, CnState* cs) {
    hipLaunchKernelGGL(k_cn_keys, dim3(grid), dim3(256), 0, h->stream, dP, rows, T, st, bound,
                       h->cn_key.p, cs);
  }
  // once, ahead of the passes: kk rows of G (m: the selected ranks)
  int targets(tcmp_handle* h, const PlanParams* dP, size_t kk, size_t m) {
    hipLaunchKernelGGL(k_cn_targets, dim3(grid_for((long long)kk, 256)), dim3(256), 0, h->stream,
                       dP, (int)kk, h->cn_to.p);
    return 0;
  }
  void pass_targets(tcmp_handle*, const PlanParams*, const double*, const int*, int, int) {}
  void pick(tcmp_handle* h, const PlanParams* dP, const double* rows, const int* ids, int r0, int n,
            const CnState* cs, DevState* st, Tree tr, long long max_nodes, CnPick* dpick) {
    hipLaunchKernelGGL(k_cn_pick, dim3(1), dim3(1024), 0, h->stream, dP, rows, ids, h->cn_nsafe.p,
                       h->cn_nsteps.p, h->cn_last.p, r0, n, cs, st, tr, max_nodes, dpick);
  }
  int finish(tcmp_handle*, size_t) { return 0; }  // copies queued ahead of the last wait
};

// The stage on T tree rows (stride 8: configuration, cost).  dP: the device copy of the goal,
// weights, resolutions, tolerance, torque mode and mass, already queued.  st, tr: the open
// plan's state and tree (the plan form; B and the node write are the device's), or null and an
// empty Tree (the stand-alone form, B = bound).  The edges' launch counts into the engine's
// scratch state.  One host wait for the counts, then one per pass.
template <class Stage>
int cn_run(tcmp_handle* h, const PlanParams* dP, const double* rows, long long T, DevState* st,
           Tree tr, long long max_nodes, double bound, int K, int passes, const CnOut* o,
           tcmp_connect_result* r, Stage& sg) {
  if (int rc = h->st_sc.ensure()) return rc;
  int rc = h->cn_state.ensure(sizeof(CnState) + sizeof(CnPick));
  rc = rc ? rc : h->cn_key.ensure((size_t)T);
  if (rc) return rc;
  CnState* cs = reinterpret_cast<CnState*>(h->cn_state.p);
  CnPick* dpick = reinterpret_cast<CnPick*>(h->cn_state.p + sizeof(CnState));
  StageSpan t(h);
  const unsigned grid = (unsigned)std::min<long long>(grid_for(T, 256), (long long)h->cu_count * 8);
  HIPCHK(hipMemsetAsync(cs, 0, sizeof(CnState), h->stream));
  HIPCHK(hipMemsetAsync(&cs->key_min, 0xFF, sizeof(cs->key_min), h->stream));
  sg.keys(h, grid, dP, rows, T, st, bound, cs);
  HIPCHK(hipGetLastError());
  CnState head{};  // (the fields ahead of the digits)
  const size_t head_bytes = offsetof(CnState, cnt);
  HIPCHK(hipMemcpyAsync(&head, cs, head_bytes, hipMemcpyDeviceToHost, h->stream));
  if (int rc_s = sync_stream(h)) return rc_s;
  const long long M = (long long)std::min<unsigned long long>(head.n_eligible,
                                                              (unsigned long long)K * passes);
  r->n_nodes = T;
  r->n_eligible = (int64_t)head.n_eligible;
  r->n_selected = M;
  r->goal_node_before = r->goal_node_after = head.goal_before;
  r->cost_before = r->cost_after = head.cost_before;
  r->parent = r->rank = -1;
  r->status = TCMP_CONNECT_NONE;
  if (head.n_eligible) memcpy(&r->key_min, &head.key_min, sizeof(double));
  if (o && (o->ids || o->keys || o->nsafe || o->nsteps || o->gidx) && o->cap < M)
    return fail(-4, "output capacity too small");
  CnPick pick{};
  if (M > 0) {
    const size_t m = (size_t)M, kk = (size_t)std::min<long long>(K, M);
    for (int b = 0; b < 2; ++b) {
      rc = rc ? rc : h->cn_skey[b].ensure(m);
      rc = rc ? rc : h->cn_sidx[b].ensure(m);
    }
    rc = rc ? rc : h->cn_nsafe.ensure(m);
    rc = rc ? rc : h->cn_nsteps.ensure(m);
    rc = rc ? rc : h->cn_to.ensure(kk * 8);
    rc = rc ? rc : h->cn_last.ensure(kk * 8);
    rc = rc ? rc : h->cn_rec.ensure(kk * 8);
    if (rc) return rc;
    unsigned long long* sk[2] = {h->cn_skey[0].p, h->cn_skey[1].p};
    unsigned* si[2] = {h->cn_sidx[0].p, h->cn_sidx[1].p};
    size_t tb0 = 0, tb1 = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tb0, si[0], si[1], sk[0], sk[1], m, 0, 32, h->stream));
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tb1, sk[1], sk[0], si[1], si[0], m, 0, 64, h->stream));
    if ((rc = h->cn_tmp.ensure(std::max(tb0, tb1)))) return rc;
    // the M-th smallest composite, unless every eligible row is wanted
    const int all = (unsigned long long)M == head.n_eligible;
    // (the edge launch indexes the tree by these rows: never uninitialised memory)
    HIPCHK(hipMemsetAsync(sk[0], 0, m * sizeof(unsigned long long), h->stream));
    HIPCHK(hipMemsetAsync(si[0], 0, m * sizeof(unsigned), h->stream));
    if (!all)
      for (int d = 0; d < kCnDigits; ++d)
        hipLaunchKernelGGL(k_cn_hist, dim3(grid), dim3(256), 0, h->stream, h->cn_key.p, T, d,
                           (unsigned long long)(M - 1), cs);
    hipLaunchKernelGGL(k_cn_compact, dim3(grid), dim3(256), 0, h->stream, h->cn_key.p, T, all,
                       (unsigned)M, cs, sk[0], si[0]);
    HIPCHK(hipGetLastError());
    // (key, index) order: stable sorts by the index, then by the key
    size_t tb = h->cn_tmp.n;
    HIPCHK(rocprim::radix_sort_pairs(h->cn_tmp.p, tb, si[0], si[1], sk[0], sk[1], m, 0, 32, h->stream));
    tb = h->cn_tmp.n;
    HIPCHK(rocprim::radix_sort_pairs(h->cn_tmp.p, tb, sk[1], sk[0], si[1], si[0], m, 0, 64, h->stream));
    const int* ids = reinterpret_cast<const int*>(si[0]);
    HIPCHK(hipMemsetAsync(h->cn_nsafe.p, 0xFF, m * sizeof(int), h->stream));  // -1: not tested
    HIPCHK(hipMemsetAsync(h->cn_nsteps.p, 0xFF, m * sizeof(int), h->stream));
    HIPCHK(hipMemsetAsync(h->st_sc, 0, sizeof(DevState), h->stream));
    if ((rc = sg.targets(h, dP, kk, m))) return rc;
    for (int p = 0; p < passes && (long long)p * K < M; ++p) {
      const int r0 = p * K, n = (int)std::min<long long>(M - r0, K);
      const EdgeJob J{rows, ids + r0, h->cn_to.p, n, h->cn_nsafe.p + r0, h->cn_nsteps.p + r0,
                      h->cn_last.p, nullptr, nullptr, h->cn_rec.p};
      sg.pass_targets(h, dP, rows, ids, r0, n);
      if ((rc = launch_edges(h, h->st_sc, J, dP))) return rc;
      sg.pick(h, dP, rows, ids, r0, n, cs, st, tr, max_nodes, dpick);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(&pick, dpick, sizeof(pick), hipMemcpyDeviceToHost, h->stream));
      if (int rc_s = sync_stream(h)) return rc_s;
      r->passes_run = p + 1;
      r->n_tested += n;
      r->n_valid += (int64_t)pick.n_valid;
      if (pick.found) break;
    }
    unsigned long long steps = 0;
    HIPCHK(hipMemcpyAsync(&steps, &h->st_sc->edge_steps, sizeof(steps), hipMemcpyDeviceToHost,
                          h->stream));
    if (o) {
      if (o->ids) rc = rc ? rc : download(h, o->ids, ids, m);
      if (o->keys) rc = rc ? rc : download(h, o->keys, sk[0], m);
      if (o->nsafe) rc = rc ? rc : download(h, o->nsafe, h->cn_nsafe.p, m);
      if (o->nsteps) rc = rc ? rc : download(h, o->nsteps, h->cn_nsteps.p, m);
      if (rc) return rc;
    }
    if ((rc = sg.finish(h, m))) return rc;
    t.end();
    if (int rc_s = sync_stream(h)) return rc_s;
    r->edge_steps = steps;
  } else {
    t.end();
    if (t.timed())
      if (int rc_s = sync_stream(h)) return rc_s;
  }
  r->ms = t.ms();
  if (pick.found) {
    r->parent = pick.parent;
    r->rank = pick.rank;
    if (pick.full) {
      r->status = TCMP_CONNECT_TREE_FULL;
    } else {
      r->status = TCMP_CONNECT_OK;
      r->cost_after = pick.c;
      r->goal_node_after = tr.cfg ? pick.node : r->goal_node_before;
      if (o && o->node) {
        memcpy(o->node, pick.last, sizeof(pick.last));
        o->node[7] = pick.c;
      }
    }
  }
  return 0;
}

// The stand-alone forms' argument checks and staging (goal: the row that goes into P.goal): the
// result cleared, then P and the rows of 8 filled and queued to h->dPx and h->cn_rows.  P and tmp
// are the caller's: the copies read them until its next wait.
int cn_stage(tcmp_handle* h, const double* nodes, const double* cost, int64_t n, const double* goal,
             double bound, const double* resolutions, const double* weights, double goal_tolerance,
             int32_t torque_mode, double payload_mass, int64_t cap_out, const tcmp_connect_cfg* cfg,
             void* res, size_t res_bytes, int* K, int* passes, PlanParams& P,
             std::vector<double>& tmp) {
  if (!nodes || !cost || !goal || !res || n < 1 || n > INT_MAX || cap_out < 0)
    return fail(-1, "bad arguments");
  if (torque_mode < 0 || torque_mode > 3) return fail(-1, "unknown torque mode");
  if (bound != bound) return fail(-1, "the bound is NaN (INFINITY: none)");
  if (int rc = cn_cfg(cfg, K, passes)) return rc;
  memset(res, 0, res_bytes);
  P = default_params();
  for (int k = 0; k < 7; ++k) {
    if (resolutions) P.res[k] = resolutions[k];
    if (weights) P.w[k] = weights[k];
    if (!(P.res[k] > 0.0) || !(P.w[k] > 0.0))
      return fail(-1, "resolutions and weights must be positive");
    P.goal[k] = goal[k];
  }
  P.goal_tol = goal_tolerance;
  P.torque_mode = torque_mode;
  P.mass = payload_mass;
  // rows of 8: the configuration, then the cost (negative costs have no ordered integer image)
  tmp.resize((size_t)n * 8);
  for (int64_t i = 0; i < n; ++i) {
    if (cost[i] < 0.0) return fail(-1, "negative node cost");
    for (int k = 0; k < 7; ++k) tmp[8 * i + k] = nodes[7 * i + k];
    tmp[8 * i + 7] = cost[i];
  }
  if (int rc = h->dPx.ensure()) return rc;
  if (int rc = upload(h, h->cn_rows, tmp.data(), tmp.size())) return rc;
  HIPCHK(hipMemcpyAsync(h->dPx, &P, sizeof(P), hipMemcpyHostToDevice, h->stream));
  return 0;
}

}  // namespace

extern "C" {

int tcmp_connect_nodes(tcmp_handle* h, const double* nodes, const double* cost, int64_t n,
                       const double* goal, double bound, const double* resolutions,
                       const double* weights, double goal_tolerance, int32_t torque_mode,
                       double payload_mass, const tcmp_connect_cfg* cfg, int32_t* ids_out,
                       double* keys_out, int32_t* nsafe_out, int32_t* nsteps_out, int64_t cap_out,
                       double* node_out, tcmp_connect_result* res) {
  TCMP_ENTER(h);
  int K, passes;
  PlanParams P;
  std::vector<double> tmp;
  if (int rc = cn_stage(h, nodes, cost, n, goal, bound, resolutions, weights, goal_tolerance,
                        torque_mode, payload_mass, cap_out, cfg, res, sizeof(*res), &K, &passes, P,
                        tmp))
    return rc;
  const CnOut o{ids_out, keys_out, nsafe_out, nsteps_out, cap_out, node_out};
  CnSingle sg;
  return cn_run(h, h->dPx, h->cn_rows.p, n, nullptr, Tree{}, 0, bound, K, passes, &o, res, sg);
}

int tcmp_plan_connect(tcmp_handle* h, const tcmp_connect_cfg* cfg, tcmp_connect_result* res) {
  TCMP_ENTER(h);
  if (!res) return fail(-1, "null result");
  if (!h->plan_open) return fail(-1, "no open plan");
  int K, passes;
  if (int rc = cn_cfg(cfg, &K, &passes)) return rc;
  memset(res, 0, sizeof(*res));
  long long T = 0;
  HIPCHK(hipMemcpyAsync(&T, &h->st->n_nodes, sizeof(T), hipMemcpyDeviceToHost, h->stream));
  if (int rc_s = sync_stream(h)) return rc_s;
  if (T < 1 || T > INT_MAX) return fail(-1, "no tree to connect");
  CnSingle sg;
  if (int rc = cn_run(h, h->dP, h->cfg.p, T, h->st, Tree{h->cfg.p, h->parent.p, h->tgt.p, h->meta.p},
                      h->P.max_nodes, INFINITY, K, passes, nullptr, res, sg))
    return rc;
  if (res->status == TCMP_CONNECT_OK) {
    // the tree has a node no round added: the host's bound on its size follows, the stored
    // shortcut list and the finished rows describe the old path
    ++h->extra_nodes;
    h->sc_live = false;
    h->fin_status = -1;
  }
  return 0;
}

}  // extern "C"
