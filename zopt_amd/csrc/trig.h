// sin and cos of one fp64 argument together, for the model code (models.h, rollout_fast.hip): the library sincos is ~150 VALU
// instructions (it carries a Payne-Hanek path for huge arguments), three of them per model evaluation.  Here:
// Cody-Waite reduction by pi/2 in two FMA steps (exact cancellation by the fused product; the neglected third term is
// k * 1.5e-33) and the minimax kernels of fdlibm's __kernel_sin / __kernel_cos on [-pi/4, pi/4] (Sun Microsystems' public
// coefficient tables): ~35 instructions.  Contract for |x| <= 1e6, with k = rint(2x/pi), asserted against 400-bit arithmetic on a
// host build of this header (tests/trig_shim.cpp, tests/test_sincos.py) and bit for bit against that build on the device
// (tests/test_sincos_gpu.py):
//     |error| <= 1.4 ulp(result) + (|k| + 1) * 1.6e-33.
// The second term is the neglected third term of pi/2.  It matters only right next to a zero of sin or cos (x = fl(k pi/2) and its
// neighbours), where the result itself is ~1e-17 |k| or smaller: there the ulp bound alone does NOT hold, at small arguments
// either (450 ulp measured for |k| <= 64, more for some larger k), while the absolute error stays near |k| * 1.5e-33.  Beyond
// 1e6 the absolute error keeps growing like 1.5e-33 |x| up to |x| ~ 2^52; past that the reduction has no meaning and the results
// need not be finite (1e300 gives inf / NaN).  +-inf and NaN give NaN.  sin(-0.0) is +0.0, not -0.0: the reduction's
// fma(-k, pi/2, x) with k = -0.0 adds +0.0 to -0.0.  Tiny and subnormal x: sin(x) = x, cos(x) = 1 exactly.
#pragma once
#include <hip/hip_runtime.h>

namespace zm {

__device__ __forceinline__ void zm_sincos(const double x, double* sn, double* cs) {
#pragma clang fp contract(off)   // every FMA below is explicit: the same bits in whichever kernel this is inlined (see quad_step.h)
    const double k = __builtin_rint(x * 6.36619772367581382433e-01);        // x * 2/pi
    double r = __builtin_fma(-k, 1.57079632679489655800e+00, x);            // fl(pi/2)
    r = __builtin_fma(-k, 6.12323399573676603587e-17, r);                   // pi/2 - fl(pi/2)
    const double z = r * r;
    // sin(r) = r + r^3 (S1 + z (S2 + ...))
    double ps = __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = __builtin_fma(z, ps, 2.75573137070700676789e-06);
    ps = __builtin_fma(z, ps, -1.98412698298579493134e-04);
    ps = __builtin_fma(z, ps, 8.33333333332248946124e-03);
    ps = __builtin_fma(z, ps, -1.66666666666666324348e-01);
    const double s = __builtin_fma(r * z, ps, r);
    // cos(r) = 1 - z/2 + z^2 (C1 + z (C2 + ...)), the leading terms summed without cancellation error
    double pc = __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = __builtin_fma(z, pc, -2.75573143513906633035e-07);
    pc = __builtin_fma(z, pc, 2.48015872894767294178e-05);
    pc = __builtin_fma(z, pc, -1.38888888888741095749e-03);
    pc = __builtin_fma(z, pc, 4.16666666666666019037e-02);
    const double hz = 0.5 * z, w = 1.0 - hz;
    const double c = w + __builtin_fma(z * z, pc, (1.0 - w) - hz);
    // quadrant k mod 4:  0: (s, c)   1: (c, -s)   2: (-s, -c)   3: (-c, s)
    const int q = (int)__builtin_fma(-4.0, __builtin_rint(0.25 * k), k);   // k mod 4 in {-2..2}, no integer overflow for huge k
    const double s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
    *sn = (q & 2) ? -s1 : s1;
    *cs = ((q + 1) & 2) ? -c1 : c1;
}

}  // namespace zm
