// Bodies held by the gripper (get_collision_fn(..., attachments=[...]), utils.py:3165-3218: the
// attached bodies are assigned to their parent link at every configuration and tested against
// every obstacle, pairwise_collision at the same -0.04 closest-point threshold).
//
// A held body is a convex hull in its own (child) frame, rigidly placed on one of the ten moving
// collision links: world_from_child(q) = world_from_parent(q) * parent_from_child.  Its depth
// against an obstacle is the minimum overlap over every candidate axis of the two hulls (facet
// normals of both, every normalised cross product of two unit edge directions, pairs with a
// squared cross norm below 1e-12 skipped), fp64 without contraction -- k_base_pd's definition.
// A box obstacle enters with its 3 axes and an analytic support, a mesh with its world-frame
// rows Scene::mv64 / mp64 / me64.  The held flag of a configuration is
// max over bodies and obstacles of depth >= kPen; no joint-limit test, no test against the
// robot's own links (utils.py:3191 is a TODO there as well) or among held bodies.
//
// One device function, att_flag, decides the flag from (cq, sq); the per-configuration kernel,
// the edge post-pass and the rewire walk all call it, so they cannot differ in a bit.  The new
// kernels run after the existing ones and only when an attachment is set: no existing kernel
// changes.
//
// Work split of k_att_edges: kAttLanes = 8 adjacent lanes share an edge and test 8 consecutive
// steps of its accepted prefix at a time, each lane regenerating its own step by the walk's own
// refine_step sequence (the same bits, as k_edges' SPLIT lanes do).  The groups take the work
// records in k_edges' own order, which a round sorts longest planned edge first, so the eight
// edges of a wave have similar lengths.  The persistent work counter of k_edges was not taken:
// the post-pass is bounded by the accepted prefix (no lane ever waits for a fetch), its per-step
// cost is a fraction of the arm's, and 8 lanes per edge cut the longest edge's latency by 8
// where a counter would only reorder whole edges.
#pragma once

constexpr int kAttMax = 4;      // held bodies
constexpr int kAttMaxV = 64;    // vertices per body: at most 124 facets and 186 edges
constexpr int kAttMaxF = 124;
constexpr int kAttMaxE = 186;
constexpr int kAttLanes = 8;    // lanes per edge in k_att_edges
constexpr unsigned kAttLdsLimit = 96u * 1024u;  // dynamic LDS the new kernels may ask for: 384
                                                // obstacle records and four largest hulls are 84 KiB
constexpr double kAttCertGuard = 1e-4;  // certificates skip only below kPen - guard (as the LODs)

struct AttBody {
  int link;        // parent: moving collision link 0..9
  int nv, nf, ne;  // vertices, facet axes, edge directions (parallel duplicates dropped)
  int v0, f0, e0;  // their first rows in AttSet::geo
  int pad;
};
struct AttSet {
  const double* geo;  // rows of 3: every body's vertices, unit facet normals, unit edge directions
  int n;              // bodies (0: none set)
  int rows;           // rows of geo
  int n_box, n_mesh;  // the scene's obstacles the bodies are tested against
  AttBody b[kAttMax];
  double pfc[kAttMax][12];   // parent_from_child: R row-major, p
  double ball[kAttMax][4];   // bounding ball in the child frame: centre, radius
};
__host__ __device__ inline unsigned att_lds_bytes(const AttSet& A) {
  return (unsigned)((A.n_box + A.n_mesh) * 16 + A.rows * 3 + 1) * (unsigned)sizeof(double);
}

// the block's LDS copy: the obstacle records (boxes, then the meshes' outer boxes) and the hulls
struct AttLds {
  const double* obs;
  const double* geo;
};
__device__ __forceinline__ AttLds att_stage(const AttSet& A, const Scene& sc_g, double* lds) {
  const int no = (A.n_box + A.n_mesh) * 16;
  for (int i = threadIdx.x; i < no; i += blockDim.x) lds[i] = sc_g.obs[i];
  double* g = lds + no;
  for (int i = threadIdx.x; i < 3 * A.rows; i += blockDim.x) g[i] = A.geo[i];
  __syncthreads();
  return AttLds{lds, g};
}

// world_from_child of body b at (cq, sq): the collision model's link frame times the placement
__device__ __forceinline__ void att_pose(const AttSet& A, int b, const double cq[7],
                                         const double sq[7], double R[9], double p[3]) {
#pragma clang fp contract(off)
  double Rl[9], pl[3];
  link_pose<true>(A.b[b].link, cq, sq, Rl, pl);
  const double* c = A.pfc[b];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      R[3 * i + j] = Rl[3 * i] * c[j] + Rl[3 * i + 1] * c[3 + j] + Rl[3 * i + 2] * c[6 + j];
    p[i] = Rl[3 * i] * c[9] + Rl[3 * i + 1] * c[10] + Rl[3 * i + 2] * c[11] + pl[i];
  }
}

// Depth of body b at pose (R, p) against obstacle o (box index, then n_box + mesh index).
// STOP: return at the first axis whose overlap is below kPen (then only "< kPen" is meaningful).
template <bool STOP>
__device__ __forceinline__ double att_pair_pd(const AttSet& A, const AttLds& L, const Scene& sc,
                                              int b, int o, const double R[9], const double p[3]) {
#pragma clang fp contract(off)
  const AttBody B = A.b[b];
  const double* av = L.geo + 3 * B.v0;
  const double* an = L.geo + 3 * B.f0;
  const double* ae = L.geo + 3 * B.e0;
  const bool box = o < A.n_box;
  // the box record c(3) X(9, columns = axes) h(3), read where it lies in LDS (an axis picked by
  // a loop index is then an address, not an indexed register array)
  const double* ob = L.obs + 16 * o;
  const double* X = ob + 3;
  int v0 = 0, v1 = 0, f0 = 0, f1 = 0, e0 = 0, e1 = 0;
  if (!box) {
    const int* r = sc.mrange + kMrange * (o - A.n_box);
    v0 = r[0]; v1 = r[1]; f0 = r[2]; f1 = r[3]; e0 = r[4]; e1 = r[5];
  }
  double best = INFINITY;
  // one candidate axis n (unit, world frame); true: stop here
  auto axis = [&](double n0, double n1, double n2) -> bool {
    // the body's range: (R^T n) . v over its child-frame vertices, plus n . p
    const double m0 = R[0] * n0 + R[3] * n1 + R[6] * n2, m1 = R[1] * n0 + R[4] * n1 + R[7] * n2,
                 m2 = R[2] * n0 + R[5] * n1 + R[8] * n2;
    const double t = n0 * p[0] + n1 * p[1] + n2 * p[2];
    double amn = INFINITY, amx = -INFINITY;
    for (int i = 0; i < B.nv; ++i) {
      const double d = m0 * av[3 * i] + m1 * av[3 * i + 1] + m2 * av[3 * i + 2];
      amn = fmin(amn, d);
      amx = fmax(amx, d);
    }
    amn += t;
    amx += t;
    double bmn, bmx;
    if (box) {
      const double cc = n0 * ob[0] + n1 * ob[1] + n2 * ob[2];
      double ext = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) ext += fabs(n0 * X[a] + n1 * X[3 + a] + n2 * X[6 + a]) * ob[12 + a];
      bmn = cc - ext;
      bmx = cc + ext;
    } else {
      bmn = INFINITY;
      bmx = -INFINITY;
      for (int i = v0; i < v1; ++i) {
        const double4 w = sc.mv64[i];
        const double d = n0 * w.x + n1 * w.y + n2 * w.z;
        bmn = fmin(bmn, d);
        bmx = fmax(bmx, d);
      }
    }
    best = fmin(best, fmin(amx - bmn, bmx - amn));
    return STOP && best < kPen;
  };
  // the body's facet normals
  for (int f = 0; f < B.nf; ++f) {
    const double a0 = an[3 * f], a1 = an[3 * f + 1], a2 = an[3 * f + 2];
    if (axis(R[0] * a0 + R[1] * a1 + R[2] * a2, R[3] * a0 + R[4] * a1 + R[5] * a2,
             R[6] * a0 + R[7] * a1 + R[8] * a2))
      return best;
  }
  // the obstacle's
  const int nfb = box ? 3 : f1 - f0;
  for (int f = 0; f < nfb; ++f) {
    double n0, n1, n2;
    if (box) {
      n0 = X[f]; n1 = X[3 + f]; n2 = X[6 + f];
    } else {
      const double4 w = sc.mp64[f0 + f];
      n0 = w.x; n1 = w.y; n2 = w.z;
    }
    if (axis(n0, n1, n2)) return best;
  }
  // edge x edge
  const int neb = box ? 3 : e1 - e0;
  for (int j = 0; j < neb; ++j) {
    double b0, b1, b2;
    if (box) {
      b0 = X[j]; b1 = X[3 + j]; b2 = X[6 + j];
    } else {
      const double* rec = sc.me64 + 16 * (size_t)(e0 + j);
      b0 = rec[9]; b1 = rec[10]; b2 = rec[11];
    }
    const double lb = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    b0 /= lb; b1 /= lb; b2 /= lb;
    for (int i = 0; i < B.ne; ++i) {
      const double c0 = ae[3 * i], c1 = ae[3 * i + 1], c2 = ae[3 * i + 2];
      const double a0 = R[0] * c0 + R[1] * c1 + R[2] * c2, a1 = R[3] * c0 + R[4] * c1 + R[5] * c2,
                   a2 = R[6] * c0 + R[7] * c1 + R[8] * c2;
      double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
      const double l2 = n0 * n0 + n1 * n1 + n2 * n2;
      if (l2 < 1e-12) continue;  // parallel edges: no axis
      const double il = 1.0 / sqrt(l2);
      if (axis(n0 * il, n1 * il, n2 * il)) return best;
    }
  }
  return best;
}

// The held flag of a configuration.  Certificate: the body lies in its bounding ball (centre w,
// radius r) and a mesh in its outer box, so on the direction from the ball's centre to the
// nearest point of the (outer) box at distance D the overlap is at most r - D, and the depth,
// the minimum over all directions, is too; a pair is skipped only when that proves
// depth < kPen - 1e-4.  A centre inside the box (D = 0) proves nothing.
__device__ __forceinline__ bool att_flag(const double cq[7], const double sq[7], const AttSet& A,
                                         const AttLds& L, const Scene& sc) {
#pragma clang fp contract(off)
  const int no = A.n_box + A.n_mesh;
  for (int b = 0; b < A.n; ++b) {
    double R[9], p[3];
    att_pose(A, b, cq, sq, R, p);
    const double* s = A.ball[b];
    double w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      w[i] = R[3 * i] * s[0] + R[3 * i + 1] * s[1] + R[3 * i + 2] * s[2] + p[i];
    const double reach = s[3] - (kPen - kAttCertGuard) + 1e-9;  // D above it: skipped
    for (int o = 0; o < no; ++o) {
      const double* ob = L.obs + 16 * o;
      const double d0 = w[0] - ob[0], d1 = w[1] - ob[1], d2 = w[2] - ob[2];
      double D2 = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double x = fabs(d0 * ob[3 + a] + d1 * ob[6 + a] + d2 * ob[9 + a]) - ob[12 + a];
        if (x > 0) D2 += x * x;
      }
      // (D = 0, the centre inside the box, proves nothing: the exact test decides)
      if (D2 > 0 && (reach < 0 || D2 > reach * reach)) continue;
      if (att_pair_pd<true>(A, L, sc, b, o, R, p) >= kPen) return true;
    }
  }
  return false;
}

// ORs the held flag into the flags k_check_configs wrote (one configuration per lane)
__global__ __launch_bounds__(256) void k_att_configs(const double* q, long long n, Scene sc_g,
                                                     AttSet A, int* collides) {
  extern __shared__ double tcmp_lds[];
  const AttLds L = att_stage(A, sc_g, tcmp_lds);
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || collides[i]) return;
  double x[7], cq[7], sq[7];
  load7(q + 8 * i, x);
#pragma unroll
  for (int k = 0; k < 7; ++k) sincos(x[k], &sq[k], &cq[k]);
  if (att_flag(cq, sq, A, L, sc_g)) collides[i] = 1;
}

// The probe: the depth of every (configuration, body, obstacle), no certificate, one per lane
__global__ __launch_bounds__(256) void k_att_pd(const double* q, long long n, Scene sc_g, AttSet A,
                                                double* pd) {
  extern __shared__ double tcmp_lds[];
  const AttLds L = att_stage(A, sc_g, tcmp_lds);
  const int no = A.n_box + A.n_mesh;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * A.n * no) return;
  const int o = (int)(t % no), b = (int)((t / no) % A.n);
  const long long i = t / ((long long)no * A.n);
  double x[7], cq[7], sq[7], R[9], p[3];
  load7(q + 8 * i, x);
#pragma unroll
  for (int k = 0; k < 7; ++k) sincos(x[k], &sq[k], &cq[k]);
  att_pose(A, b, cq, sq, R, p);
  pd[t] = att_pair_pd<false>(A, L, sc_g, b, o, R, p);
}

// The edge post-pass (launch_edges, after k_edges): per edge with nsafe > 0, the first step of
// the accepted prefix whose held flag is set ends the edge there -- nsafe' = that step, last' =
// the configuration after nsafe' refine steps from the edge's start, the state's extend steps
// those of the combined sequential walk (nsafe' + 1), the accepted count of the edge's 256-lane
// block one less when nothing is left.  nsteps is unchanged.  (pairs_* stay the arm walk's.)
// stats: [edges with an accepted prefix, shortened, removed], counted per wave.
__global__ __launch_bounds__(256) void k_att_edges(EdgeJob J, Scene sc_g, AttSet A, DevState* st,
                                                   unsigned long long* stats) {
  extern __shared__ double tcmp_lds[];
  const AttLds L = att_stage(A, sc_g, tcmp_lds);
  const int lane = lane_id(), sub = lane & (kAttLanes - 1);
  const int per_block = 256 / kAttLanes;
  const long long stride = (long long)gridDim.x * per_block;
  unsigned long long less = 0;  // extend steps the combined walk does not take
  unsigned seen = 0, cut = 0, gone = 0;
  for (long long k = (long long)blockIdx.x * per_block + threadIdx.x / kAttLanes;; k += stride) {
    if (__ballot(k < J.n) == 0) break;
    bool have = k < J.n;
    int e = 0, n = 1, ns = 0;
    double a[7], q2[7], q[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) a[i] = q2[i] = 0.0;
    if (have) {
      const double4 ra = *reinterpret_cast<const double4*>(J.rec + 8 * (size_t)k);
      const double4 rb = *reinterpret_cast<const double4*>(J.rec + 8 * (size_t)k + 4);
      a[0] = ra.x; a[1] = ra.y; a[2] = ra.z; a[3] = ra.w; a[4] = rb.x; a[5] = rb.y; a[6] = rb.z;
      e = __double2loint(rb.w);
      n = __double2hiint(rb.w);
      ns = J.nsafe[e];
      have = ns > 0;
      if (have) load7(J.to + 8 * (size_t)e, q2);
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) q[i] = a[i];
    int done = 0;  // refine steps applied to q
    int j = ns;    // the first step whose held flag is set
    for (int base = 0;; base += kAttLanes) {
      const bool go = have && base < ns && j == ns;  // uniform over the edge's lanes
      if (__ballot(go) == 0) break;
      const int s = base + sub;
      bool f = false;
      if (go && s < ns) {
        // step s tests the configuration after s + 1 refine steps
        for (; done <= s; ++done) refine_step(q, q2, n, done);
        double cq[7], sq[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) sincos(q[i], &sq[i], &cq[i]);
        f = att_flag(cq, sq, A, L, sc_g);
      }
      const uint64_t m = __ballot(f);
      const unsigned gm = (unsigned)(m >> (lane - sub)) & ((1u << kAttLanes) - 1u);
      if (go && gm) j = base + __builtin_ctz(gm);
    }
    if (have && sub == 0) {
      ++seen;
      if (j < ns) ++(j == 0 ? gone : cut);
    }
    if (have && j < ns && sub == 0) {
#pragma unroll
      for (int i = 0; i < 7; ++i) q[i] = a[i];
      for (int i = 0; i < j; ++i) refine_step(q, q2, n, i);
      store7(J.last + 8 * (size_t)e, q);
      J.nsafe[e] = j;
      if (j == 0 && J.accepted) atomicSub(&J.accepted[e >> 8], 1);
      less += (unsigned long long)((ns < n ? ns + 1 : n) - (j + 1));
    }
  }
  less = wave_sum_u64(less);
  if (lane == 0 && less) atomicAdd(&st->edge_steps, 0ull - less);
  const unsigned long long s0 = wave_sum_u64(seen), s1 = wave_sum_u64(cut), s2 = wave_sum_u64(gone);
  if (lane == 0) {
    if (s0) atomicAdd(&stats[0], s0);
    if (s1) atomicAdd(&stats[1], s1);
    if (s2) atomicAdd(&stats[2], s2);
  }
}
