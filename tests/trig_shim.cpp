// Host build of the device sine / cosine (zopt_amd/csrc/trig.h) for tests/test_sincos.py and tests/test_sincos_gpu.py: the same
// header the kernels include, compiled by g++ -ffp-contract=off (what the header's own pragma asks of clang), so that its error
// can be measured against multi-precision arithmetic without a GPU and its bits compared with the device's.
// The header says `__device__ __forceinline__` and includes <hip/hip_runtime.h>: the qualifiers are defined away here and the
// include is met by an empty file of that name on the include path (tests/trig_host.py writes it next to the build).
#define __device__
#define __forceinline__ inline
#include "trig.h"
#include "quad_step.h"

extern "C" void sc(const double* x, double* s, double* c, long n) {
    for (long i = 0; i < n; ++i) zm::zm_sincos(x[i], &s[i], &c[i]);
}

// One Euler step of the still-air quadcopter as the fast rollout kernels take it (rollout_fast.hip, rollout_quad.hip): zm_sincos of the
// three angles, then quad_euler_step_trig (quad_step.h: every FMA explicit, so this build rounds as the device does).
extern "C" void quad_step(const double* x, const double* u, double dt, double* xn, long n) {
    for (long i = 0; i < n; ++i) {
        double xi[12], ui[4], xo[12], sphi, cphi, sth, cth, spsi, cpsi;
        for (int j = 0; j < 12; ++j) xi[j] = x[i * 12 + j];
        for (int j = 0; j < 4; ++j) ui[j] = u[i * 4 + j];
        zm::zm_sincos(xi[6], &sphi, &cphi);
        zm::zm_sincos(xi[7], &sth, &cth);
        zm::zm_sincos(xi[8], &spsi, &cpsi);
        zm::quad_euler_step_trig(xi, ui, dt, sphi, cphi, sth, cth, spsi, cpsi, xo);
        for (int j = 0; j < 12; ++j) xn[i * 12 + j] = xo[j];
    }
}
