// tyre_wear.hip -- tyre wear and temperature of a lap-0 fleet, a race or the stand-alone step (include/lpvmpc.h, "Tyre wear and
// temperature"): one kernel behind the disturbances' and immediately in front of the tick's command / plant kernel, which it leaves as
// it is.  Per vehicle whose plant advances n > 0 simulator steps this tick: the sliding power P of the pre-tick plant state, the energy
// E, the wear W (on the old temperature), the temperature T, the grip factor g, and the live plant and tyre tables' words
// Cf, Cr, c_f = g * (gamma * base), gamma the disturbances' value of this tick where they are attached.  A frozen vehicle (n == 0) is
// not touched, so a vehicle's state depends on its own history alone.
// One lane per vehicle, 64-lane blocks; rows, state, base and live tables are word-major [word][B], so a wavefront's loads of one word
// coalesce.  No LDS, no register array (gated: no scratch), no track: the model reads no pose.  Only + - * fabs and selects, compiled
// with -ffp-contract=off: every product and sum is rounded on its own, and the words equal a float64 restatement bit for bit.
#include "lpvmpc_device.hpp"

namespace lpvmpc {

__device__ inline double wear_min(double a, double b) { return a < b ? a : b; }
__device__ inline double wear_max(double a, double b) { return a > b ? a : b; }

__global__ void __launch_bounds__(64) tyre_wear_kernel(WearDev d) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= d.B) return;
    const int n = d.nstep ? d.nstep[b] : d.n_fixed;
    if (n <= 0) return;                                                     // frozen: state, tables and tick count stay put
    const size_t B = d.B;
    const double *r = d.rows + b, *p = d.plant + (size_t)b * 8;
    double *s = d.state + b;
    const double k_wear = r[0], k_hot = r[B], k_heat = r[2 * B], k_cool = r[3 * B], T_amb = r[4 * B], T_opt = r[5 * B], k_temp = r[6 * B],
                 wear_slope = r[7 * B], cliff_at = r[8 * B], cliff_slope = r[9 * B], g_min = r[10 * B];
    const double lr = d.base[3 * B + b], m = d.base[4 * B + b];
    const double dl = (double)n * d.dt;
    // the sliding power: the rear slip angle's numerator behind the plant's own gate, times the last step's total lateral force
    const double vs = fabs(p[2]) > 0.2 ? fabs(-p[3] + lr * p[7]) : 0.0;
    const double F = m * fabs(p[5]);
    const double P = F * vs;
    const double E = s[5 * B] + P * dl;
    double W = s[0], T = s[B];
    const double hot = wear_max(0.0, T - T_opt);
    W = wear_min(1.0, W + ((k_wear * P) * dl) * (1.0 + k_hot * hot));       // on the old T
    T = T + dl * (k_heat * P - k_cool * (T - T_amb));
    const double dT = T - T_opt;                                            // the new T
    const double gT = 1.0 - (k_temp * dT) * dT;
    const double gW = (1.0 - wear_slope * W) - cliff_slope * wear_max(0.0, W - cliff_at);
    const double g = wear_min(1.0, wear_max(g_min, gW * gT));
    if (d.gamma) {
        const double gamma = d.gamma[b];
        d.live_p[4 * B + b] = g * (gamma * d.base[b]);
        d.live_p[5 * B + b] = g * (gamma * d.base[B + b]);
        d.live_t[3 * B + b] = g * (gamma * d.base[2 * B + b]);
    } else {
        d.live_p[4 * B + b] = g * d.base[b];
        d.live_p[5 * B + b] = g * d.base[B + b];
        d.live_t[3 * B + b] = g * d.base[2 * B + b];
    }
    s[0] = W; s[B] = T; s[2 * B] = P; s[3 * B] = g;
    s[4 * B] = s[4 * B] + 1.0;
    s[5 * B] = E;
}

hipError_t launch_tyre_wear(const WearDev &d, hipStream_t s) {
    hipLaunchKernelGGL(tyre_wear_kernel, dim3((d.B + 63) / 64), dim3(64), 0, s, d);
    return hipGetLastError();
}

}  // namespace lpvmpc
