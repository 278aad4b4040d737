// sensor_faults.hpp -- the faulted sensor stage (include/lpvmpc.h, "Sensor faults"): obs_substep of observer_device.hpp with a
// vehicle's fault row applied to the IMU, the GPS reading and its publication, and the encoder, then the shared obs_step.  Stateless:
// everything is keyed on the vehicle's own observer step k.  An all-off row leaves every word of the healthy stage as it is (the
// added terms are `+ 0.0` behind the existing `+ noise`, `* 1.0`, and selects that take the healthy value).  Includers are compiled
// with -ffp-contract=off like every includer of observer_device.hpp.
#pragma once
#include "observer_device.hpp"

namespace lpvmpc {

enum FaultWord { FLT_GPS_OUT_K0 = 0, FLT_GPS_OUT_LEN, FLT_GPS_LOSS_Z, FLT_GPS_JUMP_K0, FLT_GPS_JUMP_LEN, FLT_GPS_JUMP_DX, FLT_GPS_JUMP_DY,
                 FLT_IMU_W_BIAS, FLT_IMU_YAW_DRIFT, FLT_ENC_SCALE, FLT_ENC_OUT_K0, FLT_ENC_OUT_LEN };
static_assert(FLT_ENC_OUT_LEN + 1 == kFaultWords, "one name per word");

// vehicle b's row of the word-major table: loaded once, in front of the sub-step loop
__device__ inline void fault_row(const FaultDev &f, int b, double w[kFaultWords]) {
#pragma unroll
    for (int i = 0; i < kFaultWords; ++i) w[i] = f.rows[(size_t)i * f.B + b];
}

// k0 <= k < k0 + len; the words are integers below 2^31, so the sum is exact and len = 0 holds no k
__device__ inline bool fault_window(double k, double k0, double len) { return k >= k0 && k < k0 + len; }

// obs_substep (observer_device.hpp) with the fault row w; fseed = the fault configuration's seed ^ LPVMPC_FAULT_STREAM, fvid the
// fault configuration's global vehicle index.  os, st, kObsVeh, ov, b: as obs_substep
template <bool kObsVeh = false>
__device__ inline void obs_substep_faulted(const double *G, const ObsParams &p, long long vid, const double w[kFaultWords],
                                           unsigned long long fseed, long long fvid, double *os, const double st[8], double servo,
                                           double motor, ObsVeh<kObsVeh> ov = {}, int b = 0) {
    const double k = os[OBS_K] + 1.0;
    os[OBS_K] = k;
    const long long step = (long long)k;
    // 1. IMU: a yaw reading that drifts with time, a biased rate gyro
    const double imu_yaw = st[6] + obs_noise(p, vid, step, 0) + w[FLT_IMU_YAW_DRIFT] * (k * p.dt);
    const double imu_w = st[7] + obs_noise(p, vid, step, 1) + w[FLT_IMU_W_BIAS];
    // 2. GPS: the reading jumps inside the jump window; the beacon keeps its cadence, a lost publication leaves the hold as it is
    const bool jump = fault_window(k, w[FLT_GPS_JUMP_K0], w[FLT_GPS_JUMP_LEN]);
    const double gx0 = st[0] + obs_noise(p, vid, step, 2), gy0 = st[1] + obs_noise(p, vid, step, 3);
    const double gx = jump ? gx0 + w[FLT_GPS_JUMP_DX] : gx0, gy = jump ? gy0 + w[FLT_GPS_JUMP_DY] : gy0;
    const bool pub = os[OBS_GPS_CNT] > p.th_update;
    os[OBS_GPS_CNT] = pub ? 0.0 : os[OBS_GPS_CNT] + 1.0;
    bool lost = fault_window(k, w[FLT_GPS_OUT_K0], w[FLT_GPS_OUT_LEN]);
    if (pub && !lost && w[FLT_GPS_LOSS_Z] < 9.0) lost = obs_gauss(fseed, fvid, step, 5) > w[FLT_GPS_LOSS_Z];
    const bool take = pub && !lost;
    os[OBS_GPS_X] = take ? gx : os[OBS_GPS_X];
    os[OBS_GPS_Y] = take ? gy : os[OBS_GPS_Y];
    // 3. encoder: a slipping wheel scales the reading; inside the window the previous reading is delivered again, so `changed` is
    // false and the healthy rule (EST:733-741) reads 0 on the 41st stuck step
    const double v_read = w[FLT_ENC_SCALE] * (sqrt(st[2] * st[2] + st[3] * st[3]) + obs_noise(p, vid, step, 4));
    const double v = fault_window(k, w[FLT_ENC_OUT_K0], w[FLT_ENC_OUT_LEN]) ? os[OBS_ENC_PREV] : v_read;
    const bool changed = v != os[OBS_ENC_PREV];
    os[OBS_ENC_CNT] = changed ? 0.0 : os[OBS_ENC_CNT] + 1.0;
    os[OBS_ENC_MEAS] = changed ? v : (os[OBS_ENC_CNT] > 40.0 ? 0.0 : os[OBS_ENC_MEAS]);
    os[OBS_ENC_PREV] = v;
    // 4. EST:330-333: the start-up measurement, untouched
    const bool run = k * p.dt > 0.02;
    double y[5];
    y[0] = run ? os[OBS_ENC_MEAS] : os[0];
    y[1] = imu_w; y[2] = os[OBS_GPS_X]; y[3] = os[OBS_GPS_Y];
    y[4] = run ? imu_yaw : st[6];
    double L[30], A[36], Bm[12];
    obs_step<kObsVeh>(G, os, y, servo, motor, k, p.dt, L, A, Bm, ov, b);
#pragma unroll
    for (int i = 0; i < 5; ++i) os[OBS_Y + i] = y[i];
}

}  // namespace lpvmpc
