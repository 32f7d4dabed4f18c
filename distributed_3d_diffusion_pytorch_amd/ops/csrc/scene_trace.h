// The tracing rule of the procedural scenes, shared by the renderer
// (scene.hip, which states the rule in full) and the geometry-aware metric
// (consistency.hip).  Everything is fp64.
//
// S is an image's table in LDS with each centre replaced by the ray origin in
// the primitive's frame, A (o - c).  scene_nearest finds the nearest hit of a
// unit world direction, scene_dir turns pixel coordinates into that direction,
// scene_shade colours a hit; scene_trace is the three in the renderer's order.
#pragma once
#include "common.h"

#define SC_SLOTS 6
#define SC_WORDS 16
#define SC_ROW (SC_SLOTS * SC_WORDS)

namespace {

struct Hit {
  double t;        // ray parameter of the nearest hit (+inf: miss); |d| = 1, so also the distance
  int prim;        // slot of the hit, -1 on a miss
  int face;        // 0: ellipsoid; box: 1 + 2 ax + (sg > 0), ax / sg the entry axis and the normal's sign
  double c[3];     // colour in [0, 1] (scene_shade / scene_trace)
};

// 8 prim + face, -1 on a miss: one id per smooth piece of surface
__device__ __forceinline__ int scene_surface(const Hit& h) { return h.prim < 0 ? -1 : 8 * h.prim + h.face; }

// d = R normalize(Kinv [u, v, 1])
__device__ __forceinline__ void scene_dir(const double* Ki, const double* R, double u, double v, double d[3]) {
  double c0 = Ki[0] * u + Ki[1] * v + Ki[2];
  double c1 = Ki[3] * u + Ki[4] * v + Ki[5];
  double c2 = Ki[6] * u + Ki[7] * v + Ki[8];
  const double nrm = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
  c0 /= nrm;
  c1 /= nrm;
  c2 /= nrm;
  d[0] = R[0] * c0 + R[1] * c1 + R[2] * c2;
  d[1] = R[3] * c0 + R[4] * c1 + R[5] * c2;
  d[2] = R[6] * c0 + R[7] * c1 + R[8] * c2;
}

// The nearest hit along d (t, prim, face); n: its normal in the primitive's frame.
__device__ __forceinline__ Hit scene_nearest(const double (*S)[SC_WORDS], const double d[3], double n[3]) {
  const double d0 = d[0], d1 = d[1], d2 = d[2];
  Hit h;
  h.t = __builtin_inf();
  h.prim = -1;
  h.face = 0;
  double n0 = 0.0, n1 = 0.0, n2 = 0.0;
#pragma unroll 1      // (unrolled, both kinds of all six slots are live at once: 260 VGPRs against 112)
  for (int p = 0; p < SC_SLOTS; ++p) {
    const double* s = S[p];
    const int kind = (int)s[15];                // uniform over the block
    if (kind == 0) continue;
    const double q[3] = {s[0] * d0 + s[1] * d1 + s[2] * d2, s[3] * d0 + s[4] * d1 + s[5] * d2,
                         s[6] * d0 + s[7] * d1 + s[8] * d2};
    const double o[3] = {s[9], s[10], s[11]};
    double tt, m0, m1, m2;
    int face;
    bool hit;
    if (kind == 1) {
      const double a = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
      const double b = o[0] * q[0] + o[1] * q[1] + o[2] * q[2];
      const double c = o[0] * o[0] + o[1] * o[1] + o[2] * o[2] - 1.0;
      const double disc = b * b - a * c;
      hit = disc > 0.0;
      tt = (-b - sqrt(hit ? disc : 0.0)) / a;
      m0 = o[0] + tt * q[0];
      m1 = o[1] + tt * q[1];
      m2 = o[2] + tt * q[2];
      face = 0;
    } else {
      double tmin = -__builtin_inf(), tmax = __builtin_inf();
      int ax = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double inv = 1.0 / q[k];
        const double t1 = (-1.0 - o[k]) * inv, t2 = (1.0 - o[k]) * inv;
        const double tn = fmin(t1, t2), tf = fmax(t1, t2);
        if (tn > tmin) {
          tmin = tn;
          ax = k;
        }
        tmax = fmin(tmax, tf);
      }
      hit = tmin < tmax;
      tt = tmin;
      const double sg = q[ax] > 0.0 ? -1.0 : 1.0;
      m0 = ax == 0 ? sg : 0.0;
      m1 = ax == 1 ? sg : 0.0;
      m2 = ax == 2 ? sg : 0.0;
      face = 1 + 2 * ax + (sg > 0.0 ? 1 : 0);
    }
    if (hit && tt > 0.0 && tt < h.t) {
      h.t = tt;
      h.prim = p;
      h.face = face;
      n0 = m0;
      n1 = m1;
      n2 = m2;
    }
  }
  n[0] = n0;
  n[1] = n1;
  n[2] = n2;
  return h;
}

// Colour = albedo (0.35 + 0.65 max(0, n . l)), n = normalize(A^T n_local); a miss is white.
__device__ __forceinline__ void scene_shade(const double (*S)[SC_WORDS], Hit& h, const double n[3]) {
  h.c[0] = h.c[1] = h.c[2] = 1.0;
  if (h.prim >= 0) {
    const double* s = S[h.prim];
    const double n0 = n[0], n1 = n[1], n2 = n[2];
    double w0 = s[0] * n0 + s[3] * n1 + s[6] * n2;      // A^T n_local
    double w1 = s[1] * n0 + s[4] * n1 + s[7] * n2;
    double w2 = s[2] * n0 + s[5] * n1 + s[8] * n2;
    const double wn = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    w0 /= wn;
    w1 /= wn;
    w2 /= wn;
    const double ln = sqrt(0.3 * 0.3 + 0.2 * 0.2 + 1.0 * 1.0);
    const double ndl = w0 * (0.3 / ln) + w1 * (0.2 / ln) + w2 * (1.0 / ln);
    const double shade = 0.35 + 0.65 * fmax(ndl, 0.0);
    h.c[0] = s[12] * shade;
    h.c[1] = s[13] * shade;
    h.c[2] = s[14] * shade;
  }
}

// cam: Kinv [9], R [9]
__device__ __forceinline__ Hit scene_trace(const double (*S)[SC_WORDS], const double* cam, double u, double v) {
  double d[3], n[3];
  scene_dir(cam, cam + 9, u, v, d);
  Hit h = scene_nearest(S, d, n);
  scene_shade(S, h, n);
  return h;
}

// Inverse of diag(sx, sy, 1) K by the adjugate; ks (may be null): the scaled K itself.
__device__ __forceinline__ void scene_kinv(const double* k, double sx, double sy, double* kinv, double* ks) {
  const double a = k[0] * sx, b = k[1] * sx, c = k[2] * sx;
  const double d = k[3] * sy, e = k[4] * sy, f = k[5] * sy;
  const double g = k[6], h = k[7], i = k[8];
  const double A = e * i - f * h, B = f * g - d * i, C = d * h - e * g;
  const double det = a * A + b * B + c * C;
  const double adj[9] = {A, c * h - b * i, b * f - c * e, B, a * i - c * g, c * d - a * f, C, b * g - a * h,
                         a * e - b * d};
#pragma unroll
  for (int j = 0; j < 9; ++j) kinv[j] = adj[j] / det;
  if (ks != nullptr) {
    const double m[9] = {a, b, c, d, e, f, g, h, i};
#pragma unroll
    for (int j = 0; j < 9; ++j) ks[j] = m[j];
  }
}

// Table centre -> the origin T in the primitive's frame, A (T - c), in place.
__device__ __forceinline__ void scene_origin(double* s, const double* T) {
  const double x = T[0] - s[9], y = T[1] - s[10], z = T[2] - s[11];
  s[9] = s[0] * x + s[1] * y + s[2] * z;
  s[10] = s[3] * x + s[4] * y + s[5] * z;
  s[11] = s[6] * x + s[7] * y + s[8] * z;
}
}  // namespace
