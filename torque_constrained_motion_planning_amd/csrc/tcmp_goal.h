// tcmp_goal.h -- torque-aware goal search over the IK redundancy (tcmp_goal_search): an opt-in
// stage ahead of planning.  The reference turns a grasp pose into ONE goal configuration
// (panda_primitives.py:240-265): the first free value with any limit-valid IK solution, one of
// those at random, a body collision check, up to 25 retries, and only then the static torque
// test, which ends the query when it fails.  Here every (free value, branch) candidate of every
// pose is evaluated instead: candidate id = f * 8 + k of pose p is slot k of
// tcmp_ik(poses[p], free_q7[f]), filtered by the joint limits, the mode's torque test at rest and
// the scene's collision check, and the feasible ones come back ordered by (distance from ref, id).
// tcmp_ik reports angles in (-pi, pi] and joint 6's range reaches 3.7525: a candidate whose q6 is
// below the lower limit while q6 + 2 pi is at most the upper one is taken at that image (it is
// the only one: q6 <= -2.5307 is never inside itself), so ids keep their meaning; the limits, the
// distance, the torque and collision tests and the returned configuration all use the image.
//
// Stages (one host wait, nothing persistent, no inter-workgroup waiting anywhere):
//   k_goal_expand   the (pose, free value) rows k_ik takes, one lane each
//   k_ik            as compiled (tcmp_ik.h): the candidates are tcmp_ik's bit for bit
//   k_goal_base     panda_link0's depths (launch_base_pd) to one flag
//   k_goal_torque   one lane per slot: joint 6's image (written back to the candidate), limits,
//                   torques at rest, verdict, headroom, distance; the
//                   poses' counters (integer atomics); survivors appended to a work list
//   k_goal_collide  one survivor per lane through collides_wave; a hit clears the slot's key.
//                   The grid covers every slot; blocks past the list's device-side length return
//   k_goal_select   one workgroup per pose: the pose's feasible slots compacted IN SLOT ORDER
//                   (so the work list's order never shows), the max_out smallest (distance
//                   bits, id) keys by a radix select, written out in order
// The torque and collision stages stay apart: k_check_configs sits at 237 VGPRs and one RNE
// wants a SIMD to itself.
#pragma once

namespace {

constexpr unsigned long long kGoalNone = ~0ull;  // a slot's key while it is not feasible
constexpr double kGoal2Pi = 6.283185307179586;

// rows i = p * n_free + f of k_ik's inputs
__global__ __launch_bounds__(256) void k_goal_expand(const double* __restrict__ poses,
                                                     const double* __restrict__ free_q7,
                                                     int n_free, long long n,
                                                     double* __restrict__ xpose,
                                                     double* __restrict__ xfree) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long p = i / n_free;
  const int f = (int)(i - p * n_free);
#pragma unroll
  for (int k = 0; k < 12; ++k) xpose[12 * i + k] = poses[12 * p + k];
  xfree[i] = free_q7[f];
}

// ctl[1] = some base depth >= kPen (k_body_merge's test); q-independent
__global__ void k_goal_base(const double* __restrict__ base_pd, int n_base,
                            unsigned long long* ctl) {
  bool hit = false;
  for (int j = 0; j < n_base; ++j) hit |= base_pd[j] >= kPen;
  ctl[1] = hit ? 1ull : 0ull;
}

// One lane per slot s = (p * n_free + f) * 8 + k; lanes with k >= count[p * n_free + f] are
// idle.  refw: ref (7), weights (7).  key[s]: the distance's bits of a candidate that passes
// the limits and the torque test, else kGoalNone; head[s]: its headroom.  ctr: 4 per pose
// (solutions, in limits, torque ok, [feasible: k_goal_select's]); ctl[0]: the work list's length.
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MODE >= 2 ? 1 : 2)))
void k_goal_torque(double* __restrict__ sols, const int* __restrict__ count, int n_free,
                   long long n_slots, const double* __restrict__ refw, double mass,
                   unsigned long long* __restrict__ key, double* __restrict__ head,
                   int* __restrict__ list, unsigned long long* ctl, unsigned long long* ctr) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool in = s < n_slots;
  const long long sl = in ? s : n_slots - 1;  // (every lane stays for the ballots)
  const long long pf = sl >> 3;
  const int pose = (int)(pf / n_free);
  const bool has = in && (int)(sl & 7) < count[pf];
  double q[7];
  bool lim = false, tok = false;
  double hr = 0.0, dist = 0.0;
  if (has) {
#pragma unroll
    for (int k = 0; k < 7; ++k) q[k] = sols[7 * sl + k];
    if (q[5] < kLo[5] && q[5] + kGoal2Pi <= kHi[5]) {  // joint 6's image above pi
      q[5] += kGoal2Pi;
      sols[7 * sl + 5] = q[5];
    }
    lim = !limits_violated(q);
  }
  if (lim) {
    double cq[7], sq[7], t[6];
    const double z[7] = {0, 0, 0, 0, 0, 0, 0};
    sincos7(q, cq, sq);
    rt_torques<MODE>(mass, cq, sq, z, z, t);
    {
#pragma clang fp contract(off)
      tok = true;
      hr = INFINITY;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        tok &= !(fabs(t[j]) >= kEffort[j]);  // torque_ok's comparison: a NaN passes
        hr = fmin(hr, (kEffort[j] - fabs(t[j])) / kEffort[j]);
      }
    }
    double r[7], w[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      r[k] = refw[k];
      w[k] = refw[7 + k];
    }
    dist = distance(r, q, w);
  }
  if (in) {
    key[s] = tok ? (unsigned long long)__double_as_longlong(dist) : kGoalNone;
    if (tok) head[s] = hr;
  }
  // the poses' counters: one leader per pose present in the wave (64 consecutive slots)
  const int lane = lane_id();
  unsigned long long todo = __ballot(in);
  while (todo) {
    const int l0 = __builtin_ctzll(todo);
    const int p0 = __shfl(pose, l0);
    const bool mine = in && pose == p0;
    const unsigned long long m = __ballot(mine);
    const unsigned long long a = __popcll(__ballot(mine && has)), b = __popcll(__ballot(mine && lim)),
                             c = __popcll(__ballot(mine && tok));
    if (lane == l0) {
      if (a) atomicAdd(ctr + 4 * (long long)p0, a);
      if (b) atomicAdd(ctr + 4 * (long long)p0 + 1, b);
      if (c) atomicAdd(ctr + 4 * (long long)p0 + 2, c);
    }
    todo &= ~m;
  }
  // survivors to the work list: one atomic per wave
  const unsigned long long sv = __ballot(tok);
  if (sv) {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(ctl, (unsigned long long)__popcll(sv));
    base = __shfl(base, 0);
    if (tok) list[base + __popcll(sv & ((1ull << lane) - 1ull))] = (int)s;
  }
}

// One work-list entry per lane; LDS staged as k_check_configs stages it.  Lanes past the list's
// end stay in the wave (inactive) for collides_wave.
template <bool MESH>
__global__ __launch_bounds__(256) void k_goal_collide(const double* __restrict__ sols,
                                                      const int* __restrict__ list,
                                                      const unsigned long long* ctl, Scene sc_g,
                                                      Geo g_g, unsigned long long* key) {
  extern __shared__ double tcmp_lds[];
  const unsigned long long n = ctl[0];
  // block-uniform: a base collision leaves nothing feasible; blocks past the list have no work
  if (ctl[1] || (unsigned long long)blockIdx.x * 256ull >= n) return;
  Scene sc;
  Geo g;
  stage_lds<!MESH>(sc_g, g_g, tcmp_lds, sc, g);
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const bool act = i < n;
  const long long s = act ? list[i] : 0;
  double x[7];
  if (act) {
#pragma unroll
    for (int k = 0; k < 7; ++k) x[k] = sols[7 * s + k];
  } else {
    for (int k = 0; k < 7; ++k) x[k] = 0.5 * (kLo[k] + kHi[k]);
  }
  double cq[7], sq[7];
  for (int k = 0; k < 7; ++k) sincos(x[k], &sq[k], &cq[k]);
  StepStats ss = {0, 0, 0};
  const bool c = collides_wave<MESH>(cq, sq, act, sc, g, ss);
  if (act && c) key[s] = kGoalNone;
}

// the ordered exclusive prefix of a flag over the workgroup's 256 threads, and its total
__device__ __forceinline__ unsigned goal_block_scan(bool f, unsigned* wsum, unsigned& tot) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(f);
  __syncthreads();  // (the last scan's sums have been read)
  if (lane == 0) wsum[wave] = (unsigned)__popcll(m);
  __syncthreads();
  unsigned off = 0;
  tot = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) off += wsum[w];
    tot += wsum[w];
  }
  return off + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

// One workgroup per pose over its S = n_free * 8 slots.  (a) The feasible slots' (key, id)
// compacted in slot order: F of them.  (b) The K-th smallest key T, K = min(F, max_out), by a
// radix select over the key's 64 bits from the top (the keys are non-negative doubles' bits, so
// they order as integers); counts are LDS integer atomics.  (c) Selected: key < T, and of the
// ties key == T the first few in id order, K in all (<= 256), gathered in LDS.  (d) Each one's
// rank among the selected by (key, id) is its output row.  The first version ranked every
// feasible slot against every other (F^2 / 256 comparisons a thread): 7.2 ms of the stage's
// 7.7 ms at n_free = 4096 (F up to 4,658), 59 us at n_free = 256 (DESIGN 3 has this form's).
__global__ __launch_bounds__(256) void k_goal_select(
    const double* __restrict__ sols, const unsigned long long* __restrict__ key,
    const double* __restrict__ head, int S, int max_out, const unsigned long long* ctl,
    unsigned long long* lkey, int* lid, unsigned long long* ctr, double* __restrict__ q_out,
    double* __restrict__ d_out, double* __restrict__ h_out, int* __restrict__ id_out) {
  __shared__ unsigned wsum[4];
  __shared__ unsigned bitc[64];
  __shared__ unsigned long long sk[256];
  __shared__ int si[256];
  const int tid = threadIdx.x;
  const long long p = blockIdx.x, o = p * S;
  if (ctl[1]) {  // panda_link0 collides: ctr's feasible count stays 0, the rows stay empty
    return;
  }
  if (tid < 64) bitc[tid] = 0u;
  // (a) the feasible slots, in slot order
  unsigned F = 0;
  for (int c0 = 0; c0 < S; c0 += 256) {
    const int i = c0 + tid;
    const unsigned long long kk = i < S ? key[o + i] : kGoalNone;
    const bool f = kk != kGoalNone;
    unsigned tot;
    const unsigned off = F + goal_block_scan(f, wsum, tot);
    if (f) {
      lkey[o + off] = kk;
      lid[o + off] = i;
    }
    F += tot;
  }
  if (tid == 0) ctr[4 * p + 3] = F;
  __threadfence_block();
  __syncthreads();
  const unsigned K = F < (unsigned)max_out ? F : (unsigned)max_out;
  if (K == 0) return;
  // (b) T and the number of its ties still wanted
  unsigned long long T = kGoalNone;
  unsigned ties = 0;
  if (F > K) {
    unsigned long long prefix = 0ull;
    unsigned want = K;
    for (int b = 63; b >= 0; --b) {
      unsigned c0 = 0;
      for (unsigned e = tid; e < F; e += 256) {
        const unsigned long long k2 = lkey[o + e];
        const bool match = b == 63 || (k2 >> (b + 1)) == (prefix >> (b + 1));
        c0 += (match && !((k2 >> b) & 1ull)) ? 1u : 0u;
      }
      if (c0) atomicAdd(&bitc[b], c0);
      __syncthreads();
      const unsigned zeros = bitc[b];
      if (want > zeros) {
        want -= zeros;
        prefix |= 1ull << b;
      }
    }
    T = prefix;
    ties = want;
  }
  // (c) the selected, gathered
  unsigned seen = 0, nsel = 0;
  for (unsigned e0 = 0; e0 < F; e0 += 256) {
    const unsigned e = e0 + tid;
    const bool have = e < F;
    const unsigned long long k2 = have ? lkey[o + e] : kGoalNone;
    const bool eq = have && k2 == T;
    unsigned te, ts;
    const unsigned pe = goal_block_scan(eq, wsum, te);
    const bool sel = have && (k2 < T || (eq && seen + pe < ties));
    const unsigned ps = nsel + goal_block_scan(sel, wsum, ts);
    if (sel && ps < 256u) {
      sk[ps] = k2;
      si[ps] = lid[o + e];
    }
    seen += te;
    nsel += ts;
  }
  __syncthreads();
  if (nsel > 256u) nsel = 256u;  // (cannot happen: K <= max_out <= 256)
  // (d) rank and write
  if ((unsigned)tid < nsel) {
    const unsigned long long mk = sk[tid];
    const int mi = si[tid];
    unsigned rank = 0;
    for (unsigned j = 0; j < nsel; ++j) {
      const unsigned long long k2 = sk[j];
      rank += (k2 < mk || (k2 == mk && si[j] < mi)) ? 1u : 0u;
    }
    if (rank < (unsigned)max_out) {
      const long long row = p * max_out + rank;
      const long long s = o + mi;
#pragma unroll
      for (int k = 0; k < 7; ++k) q_out[7 * row + k] = sols[7 * s + k];
      d_out[row] = __longlong_as_double((long long)mk);
      h_out[row] = head[s];
      id_out[row] = mi;
    }
  }
}

int goal_lds_limits() {
  const struct { const void* k; unsigned b; } lim[] = {
      {(const void*)k_goal_collide<false>, stage_lds_bytes(kMaxObstacles)},
      {(const void*)k_goal_collide<true>, stage_lds_bytes_lean(kMaxObstacles)}};
  for (const auto& x : lim)
    HIPCHK(hipFuncSetAttribute(x.k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)x.b));
  return 0;
}

}  // namespace

extern "C" {

int tcmp_goal_search(tcmp_handle* h, const double* poses, int32_t n_pose, const double* free_q7,
                     int32_t n_free, const double* ref, const double* weights,
                     int32_t torque_mode, double payload_mass, int32_t max_out, double* q_out,
                     double* dist_out, double* headroom_out, int32_t* id_out,
                     tcmp_goal_stats* stats, double* ms) {
  TCMP_ENTER(h);
  if (int rc = att_refuse(h, "tcmp_goal_search")) return rc;
  if (!poses || !free_q7 || !ref || n_pose < 1 || n_free < 1 || max_out < 1 || max_out > 256)
    return fail(-1, "bad arguments");
  if ((long long)n_pose * n_free * 8 >= (1ll << 31)) return fail(-1, "n_pose * n_free * 8 >= 2^31");
  if (torque_mode < 0 || torque_mode > 3) return fail(-1, "unknown torque mode");
  const long long N = (long long)n_pose * n_free, NS = N * 8, R = (long long)n_pose * max_out;
  const int S = n_free * 8;
  int rc = h->gs_xpose.ensure((size_t)N * 12);
  rc = rc ? rc : h->gs_xfree.ensure((size_t)N);
  rc = rc ? rc : h->gs_sol.ensure((size_t)N * 56);
  rc = rc ? rc : h->gs_cnt.ensure((size_t)N);
  rc = rc ? rc : h->gs_key.ensure((size_t)NS);
  rc = rc ? rc : h->gs_head.ensure((size_t)NS);
  rc = rc ? rc : h->gs_list.ensure((size_t)NS);
  rc = rc ? rc : h->gs_lkey.ensure((size_t)NS);
  rc = rc ? rc : h->gs_lid.ensure((size_t)NS);
  rc = rc ? rc : h->gs_ctr.ensure((size_t)2 + 4 * (size_t)n_pose);
  rc = rc ? rc : h->gs_out.ensure((size_t)R * 9);
  rc = rc ? rc : h->gs_oid.ensure((size_t)R);
  if (rc) return rc;
  double* const refw = h->gs_refw_h;
  for (int k = 0; k < 7; ++k) {
    refw[k] = ref[k];
    refw[7 + k] = weights ? weights[k] : 10.0;
  }
  unsigned long long* const ctl = h->gs_ctr.p;
  unsigned long long* const ctr = ctl + 2;
  double* const oq = h->gs_out.p;
  double* const od = oq + 7 * R;
  double* const oh = od + R;
  rc = upload(h, h->gs_pose, poses, (size_t)n_pose * 12);
  rc = rc ? rc : upload(h, h->gs_free, free_q7, (size_t)n_free);
  rc = rc ? rc : upload(h, h->gs_refw, refw, 14);
  if (rc) return rc;
  StageSpan t(h);
  HIPCHK(hipMemsetAsync(ctl, 0, (2 + 4 * (size_t)n_pose) * sizeof(unsigned long long), h->stream));
  HIPCHK(hipMemsetAsync(oq, 0, (size_t)R * 9 * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(h->gs_oid.p, 0xff, (size_t)R * sizeof(int), h->stream));
  hipLaunchKernelGGL(k_goal_expand, dim3(grid_for(N, 256)), dim3(256), 0, h->stream, h->gs_pose.p,
                     h->gs_free.p, (int)n_free, N, h->gs_xpose.p, h->gs_xfree.p);
  hipLaunchKernelGGL(k_ik, dim3(grid_for(N, 256)), dim3(256), 0, h->stream, h->gs_xpose.p,
                     h->gs_xfree.p, N, h->gs_sol.p, h->gs_cnt.p);
  HIPCHK(hipGetLastError());
  if (int rc_b = launch_base_pd(h)) return rc_b;
  const int nb = h->n_box + h->n_mesh;
  if (nb) hipLaunchKernelGGL(k_goal_base, dim3(1), dim3(1), 0, h->stream, h->base_pd.p, nb, ctl);
  hipLaunchKernelGGL(TCMP_BY_MODE(k_goal_torque, torque_mode), dim3(grid_for(NS, 256)), dim3(256),
                     0, h->stream, h->gs_sol.p, h->gs_cnt.p, (int)n_free, NS, h->gs_refw.p,
                     payload_mass, h->gs_key.p, h->gs_head.p, h->gs_list.p, ctl, ctr);
  hipLaunchKernelGGL(h->mesh_kernels() ? k_goal_collide<true> : k_goal_collide<false>,
                     dim3(grid_for(NS, 256)), dim3(256), lds_bytes(h), h->stream, h->gs_sol.p,
                     h->gs_list.p, ctl, h->scene(), h->geo(), h->gs_key.p);
  hipLaunchKernelGGL(k_goal_select, dim3((unsigned)n_pose), dim3(256), 0, h->stream, h->gs_sol.p,
                     h->gs_key.p, h->gs_head.p, S, (int)max_out, ctl, h->gs_lkey.p, h->gs_lid.p,
                     ctr, oq, od, oh, h->gs_oid.p);
  HIPCHK(hipGetLastError());
  t.end();
  std::vector<unsigned long long> hc(2 + 4 * (size_t)n_pose);
  if (int rc = download(h, hc.data(), ctl, hc.size())) return rc;
  if (q_out)
    if (int rc = download(h, q_out, oq, (size_t)R * 7)) return rc;
  if (dist_out)
    if (int rc = download(h, dist_out, od, (size_t)R)) return rc;
  if (headroom_out)
    if (int rc = download(h, headroom_out, oh, (size_t)R)) return rc;
  if (id_out)
    if (int rc = download(h, id_out, h->gs_oid.p, (size_t)R)) return rc;
  if (int rc_s = sync_stream(h)) return rc_s;
  const float span = t.ms();
  if (ms) *ms = span;
  if (stats) {
    for (int p = 0; p < n_pose; ++p) {
      const unsigned long long* c = hc.data() + 2 + 4 * (size_t)p;
      tcmp_goal_stats& st = stats[p];
      st.n_solutions = (int64_t)c[0];
      st.n_in_limits = (int64_t)c[1];
      st.n_torque_ok = (int64_t)c[2];
      st.n_feasible = (int64_t)c[3];
      st.n_out = (int32_t)std::min<unsigned long long>(c[3], (unsigned long long)max_out);
      st.base_collides = (int32_t)hc[1];
    }
  }
  return 0;
}

}  // extern "C"
