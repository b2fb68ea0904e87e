// surfdisp_device.h -- what more than one unit runs of the reference's surfdisp96 and of depthkernel's model prologue, each piece
// stated once, so that the units return the same bits for the same layers (they are built with -ffp-contract=off like the rest of
// the library: an inline function here rounds as a copy of its text in the unit would).
//   host      the prologue that depends on the layer thicknesses only: the Earth flattening of a thickness stack (sphere_flatten),
//             the density factors of the two wave types (rho_factor_rayleigh, rho_factor_love) and the layers a knot touches
//             (knot_layer_ranges): disp.hip (DispCall::layers), disp_typed.hip (entry point), surfdisp.hip (host prologue)
//   both      brocher (also ti.hip), gtsolh and the start-up scan (startup): the surfdisp.hip host prologue, typed_kernel, disp.hip
//   device    the period equations (dltar1, Love; dltar4 with var, Rayleigh), the root search (getsol, nevill) and one period of
//             the period loop (period_step), the reference's operations in the reference's order in plain IEEE fp64.
//             surfdisp.hip (dazim_surfdisp96: one lane per model, layers in global arrays) and disp_typed.hip
//             (dazim_dispersion_kernels_typed: one lane per (column, variant), layers in LDS tables) instantiate them on their own
//             model type MD, which offers
//               float D(m), A(m), B(m), R(m)   thickness, Vp, Vs and density of layer m (1-based) after the Earth flattening
//               int mmax, llw                  number of layers; first solid layer (2 with a water layer on top, else 1)
//             (disp.hip keeps its tuned dltar4 and its lockstep search)
#pragma once
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

namespace dz_sd {

__device__ __forceinline__ double sgn(double x) { return copysign(1.0, x); }

struct VarOut {
  double w, cosp, a0, cpcq, cpy, cpz, cqw, cqx, xy, xz, wy, wz;
};

// var, inv/surfdisp96.f:868-985
__device__ inline void var(double p, double q, double ra, double rb, double wvno, double xka, double xkb, double dpth, VarOut &o) {
  double w = 0, x = 0, y = 0, z = 0, cosp = 0, cosq = 0, sinp, sinq, fac, pex = 0.0, sex = 0.0;
  if (wvno < xka) {
    sinp = sin(p);
    w = sinp / ra;
    x = -ra * sinp;
    cosp = cos(p);
  } else if (wvno == xka) {
    cosp = 1.0;
    w = dpth;
    x = 0.0;
  } else if (wvno > xka) {
    pex = p;
    fac = 0.0;
    if (p < 16) fac = exp(-2.0 * p);
    cosp = (1.0 + fac) * 0.5;
    sinp = (1.0 - fac) * 0.5;
    w = sinp / ra;
    x = ra * sinp;
  }
  if (wvno < xkb) {
    sinq = sin(q);
    y = sinq / rb;
    z = -rb * sinq;
    cosq = cos(q);
  } else if (wvno == xkb) {
    cosq = 1.0;
    y = dpth;
    z = 0.0;
  } else if (wvno > xkb) {
    sex = q;
    fac = 0.0;
    if (q < 16) fac = exp(-2.0 * q);
    cosq = (1.0 + fac) * 0.5;
    sinq = (1.0 - fac) * 0.5;
    y = sinq / rb;
    z = rb * sinq;
  }
  const double exa = pex + sex;
  o.a0 = 0.0;
  if (exa < 60.0) o.a0 = exp(-exa);
  o.w = w;
  o.cosp = cosp;
  o.cpcq = cosp * cosq;
  o.cpy = cosp * y;
  o.cpz = cosp * z;
  o.cqw = cosq * w;
  o.cqx = cosq * x;
  o.xy = x * y;
  o.xz = x * z;
  o.wy = w * y;
  o.wz = w * z;
}

// dltar4, inv/surfdisp96.f:767-865 with dnka (:1018-1062) and normc (:989-1014)
template <class MD>
__device__ double dltar4(const MD &M, double wvno, double omga) {
  double e[5], ee[5], ca[5][5];
  const int mmax = M.mmax;
  double omega = omga;
  if (omega < 1.0e-4) omega = 1.0e-4;
  const double wvno2 = wvno * wvno;
  double xka = omega / (double)M.A(mmax);
  double xkb = omega / (double)M.B(mmax);
  double wvnop = wvno + xka, wvnom = fabs(wvno - xka);
  double ra = sqrt(wvnop * wvnom);
  wvnop = wvno + xkb;
  wvnom = fabs(wvno - xkb);
  double rb = sqrt(wvnop * wvnom);
  double t = (double)M.B(mmax) / omega;
  double gammk = 2.0 * t * t;
  double gam = gammk * wvno2;
  double gamm1 = gam - 1.0;
  double rho1 = (double)M.R(mmax);
  e[0] = rho1 * rho1 * (gamm1 * gamm1 - gam * gammk * ra * rb);
  e[1] = -rho1 * ra;
  e[2] = rho1 * (gamm1 - gammk * ra * rb);
  e[3] = rho1 * rb;
  e[4] = wvno2 - ra * rb;
  VarOut v;
  for (int m = mmax - 1; m >= M.llw; m--) {
    const double am = (double)M.A(m), bm = (double)M.B(m);
    xka = omega / am;
    xkb = omega / bm;
    t = bm / omega;
    gammk = 2.0 * t * t;
    gam = gammk * wvno2;
    wvnop = wvno + xka;
    wvnom = fabs(wvno - xka);
    ra = sqrt(wvnop * wvnom);
    wvnop = wvno + xkb;
    wvnom = fabs(wvno - xkb);
    rb = sqrt(wvnop * wvnom);
    const double dpth = (double)M.D(m);
    rho1 = (double)M.R(m);
    const double p = ra * dpth, q = rb * dpth;
    var(p, q, ra, rb, wvno, xka, xkb, dpth, v);
    gamm1 = gam - 1.0;
    const double twgm1 = gam + gamm1, gmgmk = gam * gammk, gmgm1 = gam * gamm1, gm1sq = gamm1 * gamm1;
    const double rho2 = rho1 * rho1, a0pq = v.a0 - v.cpcq;
    ca[0][0] = v.cpcq - 2.0 * gmgm1 * a0pq - gmgmk * v.xz - wvno2 * gm1sq * v.wy;
    ca[0][1] = (wvno2 * v.cpy - v.cqx) / rho1;
    ca[0][2] = -(twgm1 * a0pq + gammk * v.xz + wvno2 * gamm1 * v.wy) / rho1;
    ca[0][3] = (v.cpz - wvno2 * v.cqw) / rho1;
    ca[0][4] = -(2.0 * wvno2 * a0pq + v.xz + wvno2 * wvno2 * v.wy) / rho2;
    ca[1][0] = (gmgmk * v.cpz - gm1sq * v.cqw) * rho1;
    ca[1][1] = v.cpcq;
    ca[1][2] = gammk * v.cpz - gamm1 * v.cqw;
    ca[1][3] = -v.wz;
    ca[1][4] = ca[0][3];
    ca[3][0] = (gm1sq * v.cpy - gmgmk * v.cqx) * rho1;
    ca[3][1] = -v.xy;
    ca[3][2] = gamm1 * v.cpy - gammk * v.cqx;
    ca[3][3] = ca[1][1];
    ca[3][4] = ca[0][1];
    ca[4][0] = -(2.0 * gmgmk * gm1sq * a0pq + gmgmk * gmgmk * v.xz + gm1sq * gm1sq * v.wy) * rho2;
    ca[4][1] = ca[3][0];
    ca[4][2] = -(gammk * gamm1 * twgm1 * a0pq + gam * gammk * gammk * v.xz + gamm1 * gm1sq * v.wy) * rho1;
    ca[4][3] = ca[1][0];
    ca[4][4] = ca[0][0];
    const double tt = -2.0 * wvno2;
    ca[2][0] = tt * ca[4][2];
    ca[2][1] = tt * ca[3][2];
    ca[2][2] = v.a0 + 2.0 * (v.cpcq - ca[0][0]);
    ca[2][3] = tt * ca[1][2];
    ca[2][4] = tt * ca[0][2];
#pragma unroll
    for (int i = 0; i < 5; i++) {
      double cr = 0.0;
#pragma unroll
      for (int j = 0; j < 5; j++) cr = cr + e[j] * ca[j][i];
      ee[i] = cr;
    }
    double t1 = 0.0;
#pragma unroll
    for (int i = 0; i < 5; i++)
      if (fabs(ee[i]) > t1) t1 = fabs(ee[i]);
    if (t1 < 1.e-40) t1 = 1.0;
#pragma unroll
    for (int i = 0; i < 5; i++) e[i] = ee[i] / t1;
  }
  if (M.llw != 1) {  // water layer on top, :844-860
    xka = omega / (double)M.A(1);
    wvnop = wvno + xka;
    wvnom = fabs(wvno - xka);
    ra = sqrt(wvnop * wvnom);
    const double dpth = (double)M.D(1);
    rho1 = (double)M.R(1);
    const double p = ra * dpth;
    const double znul = 1.0e-05;
    var(p, znul, ra, znul, wvno, xka, znul, dpth, v);
    const double w0 = -rho1 * v.w;
    return v.cosp * e[0] + w0 * e[1];
  }
  return e[0];
}

// dltar1: SH period equation, inv/surfdisp96.f:704-763
template <class MD>
__device__ double dltar1(const MD &M, double wvno, double omega) {
  const int mmax = M.mmax;
  double beta1 = (double)M.B(mmax);
  double rho1 = (double)M.R(mmax);
  double xkb = omega / beta1;
  double wvnop = wvno + xkb, wvnom = fabs(wvno - xkb);
  double rb = sqrt(wvnop * wvnom);
  double e1 = rho1 * rb;
  double e2 = 1.0 / (beta1 * beta1);
  for (int m = mmax - 1; m >= M.llw; m--) {
    beta1 = (double)M.B(m);
    rho1 = (double)M.R(m);
    const double dm = (double)M.D(m);
    const double xmu = rho1 * beta1 * beta1;
    xkb = omega / beta1;
    wvnop = wvno + xkb;
    wvnom = fabs(wvno - xkb);
    rb = sqrt(wvnop * wvnom);
    const double q = dm * rb;
    double y, z, cosq, sinq, fac;
    if (wvno < xkb) {
      sinq = sin(q);
      y = sinq / rb;
      z = -rb * sinq;
      cosq = cos(q);
    } else if (wvno == xkb) {
      cosq = 1.0;
      y = dm;
      z = 0.0;
    } else {
      fac = 0.0;
      if (q < 16) fac = exp(-2.0 * q);
      cosq = (1.0 + fac) * 0.5;
      sinq = (1.0 - fac) * 0.5;
      y = sinq / rb;
      z = rb * sinq;
    }
    const double e10 = e1 * cosq + e2 * xmu * z;
    const double e20 = e1 * y / xmu + e2 * cosq;
    double xnor = fabs(e10);
    const double ynor = fabs(e20);
    if (ynor > xnor) xnor = ynor;
    if (xnor < 1.e-40) xnor = 1.0;
    e1 = e10 / xnor;
    e2 = e20 / xnor;
  }
  return e1;
}

template <class MD>
__device__ double dltar(const MD &M, double wvno, double omega, int kk) {  // :684-700
  return kk == 1 ? dltar1(M, wvno, omega) : dltar4(M, wvno, omega);
}

constexpr double TWOPI = 2.0 * 3.141592653589793;

// nevill, inv/surfdisp96.f:551-668 (half :670-680 inlined)
template <class MD>
__device__ double nevill(const MD &M, double t, double c1, double c2, double del1, double del2, int ifunc) {
  double x[20], y[20];
  const double omega = TWOPI / t;
  double c3 = 0.5 * (c1 + c2);
  double del3 = dltar(M, omega / c3, omega, ifunc);
  int nev = 1, nctrl = 1, m = 1;
  for (;;) {
    nctrl++;
    if (nctrl >= 100) break;
    if (c3 < fmin(c1, c2) || c3 > fmax(c1, c2)) {
      nev = 0;
      c3 = 0.5 * (c1 + c2);
      del3 = dltar(M, omega / c3, omega, ifunc);
    }
    const double s13 = del1 - del3, s32 = del3 - del2;
    if (sgn(del3) * sgn(del1) < 0.0) {
      c2 = c3;
      del2 = del3;
    } else {
      c1 = c3;
      del1 = del3;
    }
    if (fabs(c1 - c2) <= 1.e-6 * c1) break;
    if (sgn(s13) != sgn(s32)) nev = 0;
    const double ss1 = fabs(del1), s1 = (double)0.01f * ss1;
    const double ss2 = fabs(del2), s2 = (double)0.01f * ss2;
    bool halve = s1 > ss2 || s2 > ss1 || nev == 0;
    if (!halve) {
      if (nev == 2) {
        x[m] = c3;
        y[m] = del3;
      } else {
        x[0] = c1;
        y[0] = del1;
        x[1] = c2;
        y[1] = del2;
        m = 1;
      }
      for (int kk = 1; kk <= m; kk++) {
        const int j = m - kk + 1;
        const double denom = y[m] - y[j - 1];
        if (fabs(denom) < 1.0e-10 * fabs(y[m])) {
          halve = true;
          break;
        }
        x[j - 1] = (-y[j - 1] * x[j] + y[m] * x[j - 1]) / denom;
      }
      if (!halve) {
        c3 = x[0];
        del3 = dltar(M, omega / c3, omega, ifunc);
        nev = 2;
        m = m + 1;
        if (m > 10) m = 10;
      }
    }
    if (halve) {
      c3 = 0.5 * (c1 + c2);
      del3 = dltar(M, omega / c3, omega, ifunc);
      nev = 1;
      m = 1;
    }
  }
  return c3;
}

// getsol, inv/surfdisp96.f:384-476; del1st is its SAVE variable
template <class MD>
__device__ int getsol(const MD &M, double t1, double &c1, double clow, double dc, double cm, float betmx, int ifunc,
                      int ifirst, double &del1st) {
  double c2, del1, del2;
  double omega = TWOPI / t1;
  del1 = dltar(M, omega / c1, omega, ifunc);
  if (ifirst == 1) del1st = del1;
  const double plmn = sgn(del1st) * sgn(del1);
  int idir = (ifirst == 1) ? 1 : (plmn >= 0.0 ? 1 : -1);
  for (;;) {
    c2 = (idir > 0) ? c1 + dc : c1 - dc;
    if (c2 <= clow) {
      idir = 1;
      c1 = clow;
      continue;
    }
    omega = TWOPI / t1;
    del2 = dltar(M, omega / c2, omega, ifunc);
    if (sgn(del1) != sgn(del2)) break;
    c1 = c2;
    del1 = del2;
    if (c1 < cm) return -1;
    if (c1 >= ((double)betmx + dc)) return -1;
  }
  c1 = nevill(M, t1, c1, c2, del1, del2, ifunc);
  if (c1 > (double)betmx) return -1;
  return 1;
}

// gtsolh, inv/surfdisp96.f:361-382, all fp32: the start value of the first search, from the slowest layer
__host__ __device__ inline float gtsolh(float a, float b) {
  float c = 0.95f * b;
  for (int i = 0; i < 5; i++) {
    const float gamma = b / a;
    const float kappa = c / b;
    const float k2 = kappa * kappa;
    const float gk2 = (gamma * kappa) * (gamma * kappa);
    const float fac1 = sqrtf(1.0f - gk2);
    const float fac2 = sqrtf(1.0f - k2);
    const float fr = (2.0f - k2) * (2.0f - k2) - 4.0f * fac1 * fac2;
    float frp = -4.0f * (2.0f - k2) * kappa + 4.0f * fac2 * gamma * gamma * kappa / fac1 + 4.0f * fac1 * kappa / fac2;
    frp = frp / b;
    c = c - fr / frp;
  }
  return c;
}

// Brocher's Vs -> Vp, rho of depthkernel (inv/CalSurfG.f90:49-53) and depthkernelTI (inv/depthkernelTI.f90:48-53), fp32 in the
// reference's order: every power by repeated multiplication, every sum from the left
__host__ __device__ __forceinline__ void brocher(float vs, float &vp, float &rho) {
  const float v2 = vs * vs, v3 = v2 * vs, v4 = v3 * vs;
  const float p = 0.9409f + 2.0947f * vs - 0.8206f * v2 + 0.2683f * v3 - 0.0251f * v4;
  const float p2 = p * p, p3 = p2 * p, p4 = p3 * p, p5 = p4 * p;
  vp = p;
  rho = 1.6612f * p - 0.4721f * p2 + 0.0671f * p3 - 0.0043f * p4 + 0.000106f * p5;
}

// start-up of surfdisp96 (:134-216): the extremal velocities of the stack and the start value of the first period's search, from
// the slowest layer.  layer(m, a, b) gives Vp and Vs of layer m = 1 .. mmax after the flattening
template <class F>
__host__ __device__ __forceinline__ void startup(int mmax, F &&layer, float &betmx, float &cc1) {
  float betmn = 1.e20f, a_mn = 1.0f, b_mn = 1.0f;
  betmx = -1.e20f;
  int jsol = 1;
  for (int m = 1; m <= mmax; m++) {
    float fa, fb;
    layer(m, fa, fb);
    if (fb > 0.01f && fb < betmn) {
      betmn = fb;
      a_mn = fa;
      b_mn = fb;
      jsol = 1;
    } else if (fb <= 0.01f && fa < betmn) {
      betmn = fa;
      a_mn = fa;
      b_mn = fb;
      jsol = 0;
    }
    if (fb > betmx) betmx = fb;
  }
  cc1 = jsol == 0 ? betmn : gtsolh(a_mn, b_mn);
  cc1 = .95f * cc1;
  cc1 = .90f * cc1;
}

// the constants of surfdisp96's period loop (:118-131, :184-185): the step of the bracket search, the relative period offset of a group
// velocity, and how far below the last root (x dc) the next search starts; `one` x dc above the previous mode's root
constexpr float ddc = 0.005f, h = 0.005f, sone = 1.500f;
constexpr double one = 1.0e-2, onea = (double)sone;

// One period of the period loop (:225-233, :270-304): the root ck at t (igr = 0) or at t / (1 + h), from the caller's start c1 and lower bound
// clow; for a group velocity the second root cb at t / (1 - h), searched from ck - onea dc with the lower bound clowb (ck where
// there is none, iret = -1 at :285), else cb = 0; val = sngl(ck) or the fp32 group velocity (:292-301).  Returns false, with the
// outputs untouched, where the first search fails: the curve ends.  del1st is getsol's SAVE variable.
template <class MD>
__device__ __forceinline__ bool period_step(const MD &M, double t1, int igr, int ifunc, int ifirst, double c1, double clow, double clowb,
                                            double dc, double cm, float betmx, double &del1st, double &ck, double &cb, float &val) {
  float t1a, t1b = 0.0f;
  if (igr > 0) {
    t1a = (float)(t1 / (double)(1.f + h));
    t1b = (float)(t1 / (double)(1.f - h));
    t1 = (double)t1a;
  } else {
    t1a = (float)t1;
  }
  int iret = getsol(M, t1, c1, clow, dc, cm, betmx, ifunc, ifirst, del1st);
  if (iret == -1) return false;
  ck = c1;
  if (igr > 0) {
    t1 = (double)t1b;
    c1 = c1 - onea * dc;
    iret = getsol(M, t1, c1, clowb, dc, cm, betmx, ifunc, 0, del1st);
    if (iret == -1) c1 = ck;
  } else {
    c1 = 0.0;
  }
  cb = c1;
  const float cc0 = (float)ck;
  const float cc1 = (float)c1;
  if (igr == 0) {
    val = cc0;
  } else {
    val = (1 / t1a - 1 / t1b) / (1 / (t1a * cc0) - 1 / (t1b * cc1));
  }
  return true;
}

// ---- host: the part of the prologue that depends on the layer thicknesses only, with the host libm's log / powf the reference calls ----

// sphere(0,0), inv/surfdisp96.f:132, :510-530: the thicknesses d [mmax] of a spherical stack of radius ar become those of the flat one, in
// place; tmp [mmax] receives the factor (ar+ar)/(r0+r1) that scales a layer's velocities (:528) and enters its density factor.
// The half-space counts with the dummy thickness 1 (:513) and ends with 0 (:545).
inline void sphere_flatten(int mmax, double ar, float *d, double *tmp) {
  double dr = 0.0, r0 = ar;
  d[mmax - 1] = 1.0f;
  for (int i = 0; i < mmax; i++) {
    dr = dr + (double)d[i];
    const double r1 = ar - dr;
    const double z0 = ar * log(ar / r0), z1 = ar * log(ar / r1);
    d[i] = (float)(z1 - z0);
    tmp[i] = (ar + ar) / (r0 + r1);
    r0 = r1;
  }
  d[mmax - 1] = 0.0f;
}

// sphere(ifunc,1), :169, :536-545: what a layer's density is multiplied by, btp = sngl(tmp)
inline float rho_factor_rayleigh(double tmp) { return powf((float)tmp, -2.275f); }   // btp**(-2.275), :541
inline float rho_factor_love(double tmp) {   // btp**(-5), :539: reciprocal of the integer power, as the reference's build forms it
  const float x = (float)tmp;
  const float x2 = x * x;
  return 1.0f / (x2 * x2 * x);
}

// Per knot pi = 1 .. nz the contiguous range of refined layers (anything with the interval iv of dz_refine_layers) it touches -- the
// sublayers of intervals pi - 1 and pi, for the last knot those of the last interval and the half-space --: krange [nz + 1][2] = first
// layer (1-based) and number of layers, row 0 = none.  Returns the longest range.
template <class L>
inline int knot_layer_ranges(const std::vector<L> &lay, int nz, int *krange) {
  const int mmax = (int)lay.size();
  int longest = 0;
  krange[0] = krange[1] = 0;
  for (int pi = 1; pi <= nz; pi++) {
    int lo = 0, hi = 0;
    for (int m = 1; m <= mmax; m++)
      if ((pi > 1 && lay[m - 1].iv == pi - 1) || lay[m - 1].iv == pi || (pi == nz && lay[m - 1].iv == 0)) {
        if (!lo) lo = m;
        hi = m;
      }
    krange[2 * pi] = lo, krange[2 * pi + 1] = lo ? hi - lo + 1 : 0;
    if (krange[2 * pi + 1] > longest) longest = krange[2 * pi + 1];
  }
  return longest;
}

}  // namespace dz_sd
