// The flow-matching table row and the drift it gives, shared by the fixed-grid steps (solver_steps.hip) and the adaptive
// Runge-Kutta stages (ode_adaptive.hip).  Both files are built with -ffp-contract=off: every operation rounds on its own.
#pragma once
#include "common.h"

struct FlowRow {
    float a, s, da, ds, hg2, s2, den, vden;
};
__device__ __forceinline__ FlowRow flow_row(const float* r) {
    FlowRow f;
    f.a = r[0]; f.s = r[1]; f.da = r[2]; f.ds = r[3]; f.hg2 = r[5]; f.s2 = r[6]; f.den = r[7]; f.vden = r[8];
    return f;
}
// _flow_fields + the drift: mean_type 0 START_X, 1 EPSILON, 2 VELOCITY, 3 VECTOR; sde: v - (g2/2) * score, else v.
__device__ __forceinline__ float flow_drift(const FlowRow& f, int mt, bool sde, float o, float xt) {
    float v, score = 0.f;
    if (mt == 0) {
        const float r = xt - f.a * o;
        const float eps = r / f.s;
        if (sde) score = (-r) / f.s2;
        v = f.da * o + f.ds * eps;
    } else if (mt == 1) {
        const float x0 = (xt - f.s * o) / f.a;
        if (sde) score = (-o) / f.s;
        v = f.da * x0 + f.ds * o;
    } else if (mt == 2) {
        const float x0 = (f.a * xt - f.s * o) / f.den;
        const float eps = (f.s * xt + f.a * o) / f.den;
        if (sde) score = (-eps) / f.s;
        v = f.da * x0 + f.ds * eps;
    } else {
        if (sde) score = (-((f.da * xt - f.a * o) / f.vden)) / f.s;
        v = o;
    }
    return sde ? v - f.hg2 * score : v;
}
