// tcmp_shortcut.h -- force-aware path shortcutting (tcmp_shortcut_path, tcmp_plan_shortcut): an
// opt-in stage between the retrace and min-jerk.  The batched frontier returns a handful of long
// random chords (shallow trees), and the reference loop never improves goal_n.cost once the goal
// is found (rrt_star.py:183-198 rewires the newest node only), so the path is straightened
// afterwards: every chord between the anchors of the waypoint list goes through the tree edges'
// own check (launch_edges: safe_path_force_aware(extend(from, to)), static torque test), and a
// dynamic program picks the cheapest anchor subsequence.  Deterministic, no RNG.
//
// One pass over a list W[0..n-1] (DESIGN §3 restates it; tests/shortcut_ref.py is the oracle):
//   anchors   a_k = min(k s, n - 1), s = 1 if n <= A_max else ceil((n - 1) / (A_max - 1))
//   orig[k]   the summed distance fn over the original points a_k .. a_{k+1}, left to right
//   chords    every anchor pair k < l with a_l - a_k >= 2; valid iff its whole extend is safe
//             and ends within 1e-6 of W[a_l] (the rewire acceptance, rrt_star.py:191)
//   DP        cost[l] = min(cost[l-1] + orig[l-1], min over valid k of cost[k] + dist(a_k, a_l)),
//             k ascending, strict <: the original hop wins ties, then the lowest k
//   splice    original hops copied, chords regenerated with refine_step (as k_retrace does
//             for tree edges), each ending in W[a_l] itself
// Chord e of the pair (k, l) sits at row(l) (row(l) - 1) / 2 + k, row(l) = l - (s == 1): the
// pairs of stride 1 start at l - k = 2, and with s >= 2 only the last anchor can sit one point
// behind its predecessor, which shortens the last row alone.
#pragma once

namespace {

constexpr int kScMaxAnchors = 1024;  // k_sc_dp: one anchor per thread of its block

struct ScGrid {
  long long n;     // waypoints
  long long s;     // anchor stride
  int A;           // anchors
  int C;           // chords
  int shift;       // s == 1: row(l) = l - 1
  int last_cnt;    // chords ending at the last anchor
};

// one pass's outcome (k_sc_dp, k_sc_splice)
struct ScStats {
  long long n_after;
  unsigned long long valid, used;
  double cost_before, cost_after;
  int hops;
  int overflow;
};

ScGrid sc_grid(long long n, int a_max) {
  ScGrid g{};
  g.n = n;
  g.s = n <= a_max ? 1 : (n - 1 + a_max - 2) / (a_max - 1);
  g.A = (int)((n - 1 + g.s - 1) / g.s) + 1;
  g.shift = g.s == 1;
  if (g.A >= 2) {
    const int l = g.A - 1;
    const long long gap = (n - 1) - std::min<long long>((long long)(l - 1) * g.s, n - 1);
    g.last_cnt = gap >= 2 ? l : l - 1;
    const long long m = l - g.shift;
    g.C = (int)(m * (m - 1) / 2 + g.last_cnt);
  }
  return g;
}

__device__ __forceinline__ long long sc_anchor(const ScGrid& g, int k) {
  const long long v = (long long)k * g.s;
  return v < g.n - 1 ? v : g.n - 1;
}

// ------------------------------------------------------------------------------------------
// k_sc_chords: chord e -> its anchor pair, its from / to rows as EdgeJob reads them, its
// length; thread e < A - 1 also sums original hop e
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sc_chords(const PlanParams* __restrict__ Pd,
                                                   const double* __restrict__ wp, ScGrid g,
                                                   double* from, double* to, int2* kl, double* len,
                                                   double* orig) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  double w[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) w[k] = Pd->w[k];
  if (e < g.C) {
    // row m holds m chords (the last one maybe one fewer): m (m - 1) / 2 <= e < m (m + 1) / 2
    long long m = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)e)) * 0.5);
    while (m * (m - 1) / 2 > e) --m;
    while (m * (m + 1) / 2 <= e) ++m;
    const int k = (int)(e - m * (m - 1) / 2), l = (int)m + g.shift;
    double a[7], b[7];
    load7u(wp + 7 * sc_anchor(g, k), a);
    load7u(wp + 7 * sc_anchor(g, l), b);
    store7(from + 8 * (size_t)e, a);
    store7(to + 8 * (size_t)e, b);
    from[8 * (size_t)e + 7] = 0.0;
    to[8 * (size_t)e + 7] = 0.0;
    kl[e] = make_int2(k, l);
    len[e] = distance(a, b, w);
  }
  if (e < g.A - 1) {
    const long long t0 = sc_anchor(g, e), t1 = sc_anchor(g, e + 1);
    double a[7], b[7], acc = 0.0;
    load7u(wp + 7 * t0, a);
    for (long long t = t0; t < t1; ++t) {
      load7u(wp + 7 * (t + 1), b);
      acc += distance(a, b, w);
#pragma unroll
      for (int k = 0; k < 7; ++k) a[k] = b[k];
    }
    orig[e] = acc;
  }
}

// ------------------------------------------------------------------------------------------
// k_sc_dp: one block.  The chords' verdicts (an invalid chord's length becomes +inf), then the
// dynamic program -- l sequential, k across the lanes, the DPP wave minimum on (value, k) and
// the waves' minima scanned in order, so ties go to the lowest k as in the ascending strict
// scan -- and the chosen hops, start to goal: (anchor k, chord index or -1 for the original
// hop k -> k + 1).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_sc_dp(const PlanParams* __restrict__ Pd,
                                                const double* __restrict__ wp, ScGrid g,
                                                const int2* __restrict__ kl,
                                                const int* __restrict__ nsafe,
                                                const int* __restrict__ nsteps,
                                                const double* __restrict__ last, double* len,
                                                const double* __restrict__ orig, int2* hops,
                                                ScStats* out) {
#pragma clang fp contract(off)
  __shared__ double cost[kScMaxAnchors];
  __shared__ int pred[kScMaxAnchors];
  __shared__ double wm[16];
  __shared__ int wk[16];
  __shared__ unsigned long long s_valid;
  const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  double w[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) w[k] = Pd->w[k];
  if (tid == 0) {
    s_valid = 0;
    cost[0] = 0.0;
    pred[0] = -1;
  }
  __syncthreads();
  unsigned long long nv = 0;
  for (int e = tid; e < g.C; e += 1024) {
    bool ok = nsafe[e] == nsteps[e];
    if (ok) {
      double tq[7], lq[7];
      load7u(wp + 7 * sc_anchor(g, kl[e].y), tq);
      load7(last + 8 * (size_t)e, lq);
      ok = distance(tq, lq, w) < 1e-6;
    }
    if (ok) ++nv;
    else len[e] = INFINITY;
  }
  nv = wave_sum_u64(nv);
  if (lane == 0 && nv) atomicAdd(&s_valid, nv);
  __syncthreads();  // (one block: its writes to len are visible to all its threads from here)
  double before = 0.0;
  for (int l = 1; l < g.A; ++l) {
    const long long m = l - g.shift;
    const int cnt = l == g.A - 1 ? g.last_cnt : (int)m;
    double v = INFINITY;
    if (tid < cnt) v = cost[tid] + len[m * (m - 1) / 2 + tid];
    const double mn = wave_min(v);
    const int wi = wave_min_int(v == mn ? tid : INT_MAX);
    if (lane == 0) {
      wm[wave] = mn;
      wk[wave] = wi;
    }
    __syncthreads();
    if (tid == 0) {
      const double o = orig[l - 1];
      before += o;
      double best = cost[l - 1] + o;
      int pk = -1;
      for (int q = 0; q < 16; ++q)
        if (wm[q] < best) {
          best = wm[q];
          pk = wk[q];
        }
      cost[l] = best;
      pred[l] = pk;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int H = 0;
    for (int l = g.A - 1; l > 0; l = pred[l] < 0 ? l - 1 : pred[l]) ++H;
    unsigned long long used = 0;
    int i = H;
    for (int l = g.A - 1; l > 0;) {
      const int pk = pred[l];
      if (pk < 0) {
        hops[--i] = make_int2(l - 1, -1);
        l = l - 1;
      } else {
        const long long m = l - g.shift;
        hops[--i] = make_int2(pk, (int)(m * (m - 1) / 2 + pk));
        ++used;
        l = pk;
      }
    }
    out->hops = H;
    out->used = used;
    out->valid = s_valid;
    out->cost_before = before;
    out->cost_after = g.A > 0 ? cost[g.A - 1] : 0.0;
    out->overflow = 0;
  }
}

// ------------------------------------------------------------------------------------------
// k_sc_splice: the new list from the chosen hops, one hop per thread and a prefix sum of their
// point counts (as k_retrace's), then k_retrace's tail on the new length.  One block.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sc_splice(const PlanParams* __restrict__ Pd, DevState* st,
                                                   const double* __restrict__ wp, ScGrid g,
                                                   const int2* __restrict__ hops,
                                                   const int2* __restrict__ kl,
                                                   const int* __restrict__ nsteps, double* out,
                                                   long long out_cap, ScStats* stats) {
  __shared__ long long part[256];
  const int tid = threadIdx.x;
  const int H = stats->hops;
  long long run = 1;  // waypoint 0
  for (int b0 = 0; b0 < H; b0 += 256) {
    const int i = b0 + tid;
    long long cnt = 0;
    int2 hp = make_int2(0, -1);
    if (i < H) {
      hp = hops[i];
      cnt = hp.y < 0 ? sc_anchor(g, hp.x + 1) - sc_anchor(g, hp.x) : (long long)nsteps[hp.y];
    }
    part[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const long long v = tid >= o ? part[tid - o] : 0;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    const long long off = run + part[tid] - cnt;
    if (i < H && off + cnt <= out_cap) {
      if (hp.y < 0) {
        const long long t0 = sc_anchor(g, hp.x);
        for (long long t = 1; t <= cnt; ++t) {
          double q[7];
          load7u(wp + 7 * (t0 + t), q);
          store7(out + 7 * (off + t - 1), q);
        }
      } else {
        double q[7], tq[7];
        load7u(wp + 7 * sc_anchor(g, hp.x), q);
        load7u(wp + 7 * sc_anchor(g, kl[hp.y].y), tq);
        const int ns = (int)cnt;
        for (int t = 0; t < ns - 1; ++t) {
          refine_step(q, tq, ns, t);
          store7(out + 7 * (off + t), q);
        }
        store7(out + 7 * (off + ns - 1), tq);
      }
    }
    run += part[255];
    __syncthreads();
  }
  if (tid == 0) {
    double q0[7];
    load7u(wp, q0);
    if (out_cap >= 1) store7(out, q0);
    stats->n_after = run;
    st->W = run;
    if (run > out_cap) {
      stats->overflow = 1;
      st->status = -3;
      return;
    }
    // k_retrace's tail (dynam_fn: num_intervals = move_time * 1000 / len(path))
    const long long ni = (long long)(Pd->exec_time * 1000.0 / (double)run);
    st->ni = ni;
    st->K = ni > 0 ? (run - 1) * ni : 0;
    st->first_fail = -1;
    // The status describes the new list: one the retrace found too long for an interval per
    // segment may now be short enough, and an earlier finish's validation verdict was the
    // unshortened list's.
    st->status = ni <= 0 ? TCMP_PLAN_MINJERK_ASSERT : 0;
  }
}

// The passes over the list in bufs[*cur] (rows of 7): each pass reads one buffer and writes the
// other; *cur names the buffer holding the result.  P: the distance weights, the extend
// resolutions, the torque mode and the payload mass of the chord checks (and the execution time
// of the tail); st: the state k_sc_splice's tail writes (null: the engine's scratch state).  The
// chords' launch counts into that scratch state, so a plan's counters stay its own.  One host
// wait per pass.
int sc_run(tcmp_handle* h, const PlanParams& P, DevState* st, double* const bufs[2],
           const long long caps[2], int* cur, long long n, int a_max, int passes,
           tcmp_shortcut_result* r) {
  if (int rc = h->st_sc.ensure()) return rc;
  if (!st) st = h->st_sc;
  if (int rc = h->sc_stats.ensure(sizeof(ScStats))) return rc;
  ScStats* dstats = reinterpret_cast<ScStats*>(h->sc_stats.p);
  HIPCHK(hipMemcpyAsync(h->dPx, &P, sizeof(P), hipMemcpyHostToDevice, h->stream));
  StageSpan t(h);
  r->n_before = r->n_after = n;
  for (int p = 0; p < passes; ++p) {
    const ScGrid g = sc_grid(n, a_max);
    const size_t C = (size_t)std::max(g.C, 1), A = (size_t)std::max(g.A, 1);
    int rc = h->sc_from.ensure(C * 8);
    rc = rc ? rc : h->sc_to.ensure(C * 8);
    rc = rc ? rc : h->sc_last.ensure(C * 8);
    rc = rc ? rc : h->sc_rec.ensure(C * 8);
    rc = rc ? rc : h->sc_len.ensure(C);
    rc = rc ? rc : h->sc_orig.ensure(A);
    rc = rc ? rc : h->sc_nsafe.ensure(C);
    rc = rc ? rc : h->sc_nsteps.ensure(C);
    rc = rc ? rc : h->sc_kl.ensure(C);
    rc = rc ? rc : h->sc_hops.ensure(A);
    if (rc) return rc;
    const double* in = bufs[*cur];
    double* out = bufs[*cur ^ 1];
    HIPCHK(hipMemsetAsync(h->st_sc, 0, sizeof(DevState), h->stream));
    hipLaunchKernelGGL(k_sc_chords, dim3(grid_for(std::max(g.C, g.A - 1), 256)), dim3(256), 0,
                       h->stream, h->dPx, in, g, h->sc_from.p, h->sc_to.p, h->sc_kl.p, h->sc_len.p,
                       h->sc_orig.p);
    if (g.C > 0) {
      const EdgeJob J{h->sc_from.p, nullptr, h->sc_to.p, g.C, h->sc_nsafe.p, h->sc_nsteps.p,
                      h->sc_last.p, nullptr, nullptr, h->sc_rec.p};
      if ((rc = launch_edges(h, h->st_sc, J, h->dPx))) return rc;
    }
    hipLaunchKernelGGL(k_sc_dp, dim3(1), dim3(1024), 0, h->stream, h->dPx, in, g, h->sc_kl.p,
                       h->sc_nsafe.p, h->sc_nsteps.p, h->sc_last.p, h->sc_len.p, h->sc_orig.p,
                       h->sc_hops.p, dstats);
    hipLaunchKernelGGL(k_sc_splice, dim3(1), dim3(256), 0, h->stream, h->dPx, st, in, g,
                       h->sc_hops.p, h->sc_kl.p, h->sc_nsteps.p, out, caps[*cur ^ 1], dstats);
    HIPCHK(hipGetLastError());
    ScStats s{};
    unsigned long long steps = 0;
    HIPCHK(hipMemcpyAsync(&s, dstats, sizeof(s), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&steps, &h->st_sc->edge_steps, sizeof(steps), hipMemcpyDeviceToHost,
                          h->stream));
    if (int rc_s = sync_stream(h)) return rc_s;
    if (s.overflow) return fail(-3, "waypoint capacity exceeded");
    *cur ^= 1;
    if (p == 0) {
      r->n_anchors = g.A;
      r->cost_before = s.cost_before;
    }
    r->passes_run = p + 1;
    r->n_after = n = s.n_after;
    r->cost_after = s.cost_after;
    r->chords_tested += (uint64_t)g.C;
    r->chords_valid += s.valid;
    r->chords_used += s.used;
    r->chord_steps += steps;
    if (s.used == 0) break;
  }
  t.end();
  if (t.timed()) {
    if (int rc_s = sync_stream(h)) return rc_s;
    r->ms = t.ms();
  }
  return 0;
}

int sc_cfg(const tcmp_shortcut_cfg* cfg, int* a_max, int* passes) {
  *a_max = cfg && cfg->max_anchors ? cfg->max_anchors : 512;
  *passes = cfg && cfg->passes ? cfg->passes : 1;
  if (*a_max < 2 || *a_max > kScMaxAnchors) return fail(-1, "max_anchors outside [2, 1024]");
  if (*passes < 1 || *passes > 8) return fail(-1, "passes outside [1, 8]");
  return 0;
}

}  // namespace

extern "C" {

int tcmp_shortcut_path(tcmp_handle* h, const double* waypoints, int64_t n_wp,
                       const double* resolutions, const double* weights, int32_t torque_mode,
                       double payload_mass, const tcmp_shortcut_cfg* cfg, double* out,
                       int64_t cap_out, tcmp_shortcut_result* res) {
  TCMP_ENTER(h);
  if (!waypoints || !res || n_wp < 1 || n_wp > INT_MAX || cap_out < 0 || (cap_out > 0 && !out))
    return fail(-1, "bad arguments");
  if (torque_mode < 0 || torque_mode > 3) return fail(-1, "unknown torque mode");
  int a_max, passes;
  if (int rc = sc_cfg(cfg, &a_max, &passes)) return rc;
  memset(res, 0, sizeof(*res));
  PlanParams P = default_params();
  for (int k = 0; k < 7; ++k) {
    if (resolutions) P.res[k] = resolutions[k];
    if (weights) P.w[k] = weights[k];
    if (!(P.res[k] > 0.0) || !(P.w[k] > 0.0)) return fail(-1, "resolutions and weights must be positive");
  }
  P.torque_mode = torque_mode;
  P.mass = payload_mass;
  // Rows the new list can take: a chord has int(rho) + 1 points, rho = |diff / res|, at most the
  // summed rho of the hops it replaces plus one; one more chord per anchor and pass at the most
  double rho = 0.0;
  for (int64_t t = 0; t + 1 < n_wp; ++t) {
    double s2 = 0.0;
    for (int k = 0; k < 7; ++k) {
      const double x = (waypoints[7 * (t + 1) + k] - waypoints[7 * t + k]) / P.res[k];
      s2 += x * x;
    }
    rho += std::sqrt(s2);
  }
  if (!(rho < 1e9)) return fail(-1, "waypoints too far apart for the resolutions");
  const long long cap = n_wp + (long long)rho + (long long)kScMaxAnchors * passes + 16;
  int rc = h->sc_wp[0].ensure((size_t)cap * 7);
  rc = rc ? rc : h->sc_wp[1].ensure((size_t)cap * 7);
  if (rc) return rc;
  if ((rc = upload(h, h->sc_wp[0], waypoints, (size_t)n_wp * 7))) return rc;
  double* const bufs[2] = {h->sc_wp[0].p, h->sc_wp[1].p};
  const long long caps[2] = {cap, cap};
  int cur = 0;
  // (the tail's plan fields go to the scratch state: no plan is touched)
  if ((rc = sc_run(h, P, nullptr, bufs, caps, &cur, n_wp, a_max, passes, res))) return rc;
  if (res->n_after > cap_out) return fail(-4, "output capacity too small");
  if ((rc = download(h, out, bufs[cur], (size_t)res->n_after * 7))) return rc;
  return sync_stream(h);
}

int tcmp_plan_shortcut(tcmp_handle* h, const tcmp_shortcut_cfg* cfg, tcmp_shortcut_result* res) {
  TCMP_ENTER(h);
  if (!res) return fail(-1, "null result");
  if (!h->plan_open) return fail(-1, "no open plan");
  int a_max, passes;
  if (int rc = sc_cfg(cfg, &a_max, &passes)) return rc;
  memset(res, 0, sizeof(*res));
  h->sc_live = false;
  h->fin_status = -1;  // the state describes the new list from here, not the finished rows
  hipLaunchKernelGGL(k_retrace, dim3(1), dim3(256), 0, h->stream, h->dP, h->st,
                     Tree{h->cfg.p, h->parent.p, h->tgt.p, h->meta.p}, h->chain.p, h->wp.p,
                     (long long)(h->wp.n / 7));
  HIPCHK(hipGetLastError());
  DevState& s = h->pin()->st;
  HIPCHK(hipMemcpyAsync(&s, h->st, sizeof(DevState), hipMemcpyDeviceToHost, h->stream));
  if (int rc_s = sync_stream(h)) return rc_s;
  if (s.goal_node < 0) {
    res->status = TCMP_PLAN_NO_GOAL;
    return 0;
  }
  if (s.status == -3) return fail(-3, "waypoint capacity exceeded");
  const long long n = s.W;
  // every hop of a retraced list is one extend step (rho < 1), so a pass adds at most one row
  // per chord it uses
  const long long cap1 = 2 * n + (long long)kScMaxAnchors * passes + 16;
  if (int rc = h->sc_wp[1].ensure((size_t)cap1 * 7)) return rc;
  double* const bufs[2] = {h->wp.p, h->sc_wp[1].p};
  const long long caps[2] = {(long long)(h->wp.n / 7), cap1};
  int cur = 0;
  PlanParams P = h->P;
  if (int rc = sc_run(h, P, h->st, bufs, caps, &cur, n, a_max, passes, res)) return rc;
  if (cur == 1) {
    if (res->n_after > caps[0]) return fail(-3, "waypoint capacity exceeded");
    HIPCHK(hipMemcpyAsync(h->wp.p, bufs[1], (size_t)res->n_after * 7 * sizeof(double),
                          hipMemcpyDeviceToDevice, h->stream));
    if (int rc_s = sync_stream(h)) return rc_s;
  }
  h->sc_live = true;
  return 0;
}

}  // extern "C"
