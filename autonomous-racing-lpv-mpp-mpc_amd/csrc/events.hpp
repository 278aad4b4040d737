// events.hpp -- the race event log (include/lpvmpc.h, "Race event log"; lpvmpc_race_events, lpvmpc_event_step_batch): its kernel
// arguments and the device function of one tick.  The function stands here once and is instantiated twice by events.hip, by the
// race's launch (slots in the ring) and by the batch form (slots from index 0 of the caller's arrays).  It reads what the race, the
// heats and the walls wrote on this tick and writes the log's own buffers only.
//
// One workgroup of kEventBlock threads walks the vehicles in chunks of its width, three times.  Pass 1 counts each vehicle's events
// (a PASS needs a walk over its heat's members) and sums the tick's count n, which the ring's write rule needs before the first
// event is written.  Pass 2 takes the exclusive prefix sum of the counts over the vehicle index -- 64 lanes with __shfl_up, the
// wavefronts' sums through LDS, a running base from chunk to chunk -- and writes each vehicle's events at its offset, in kind order,
// and its carry.  Pass 3, behind a barrier, stores the "before" POSITION and CLASS words: a PASS walk reads those of OTHER
// vehicles, so none may change while a walk of this tick can still read it; with one workgroup a barrier is all that takes.  No
// atomics, and nothing depends on how workgroups are scheduled.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lpvmpc.h"

namespace lpvmpc {

constexpr int kEventBlock = 1024;             // the scanning workgroup's width

// what a tick reads of the race and of the other attachments: passed at every launch, the log keeps none of it
struct EventSrc {               // passed by value
    const int32_t *phase, *lap;                 // [B]
    const int32_t *lap_step;                    // [B][lap_cols] (race form), or null
    int lap_cols;
    const double *lap_value;                    // [B] the V0 of a LAP event (batch form), or null
    // the heats' output planes and member lists; heat_f null: no heats
    const double *heat_f;                       // [LPVMPC_HEAT_F64][B]
    const int32_t *heat_i;                      // [LPVMPC_HEAT_I32][B]
    const int32_t *heat_of;                     // [B] heat of each vehicle, -1: none
    const int32_t *off, *members;               // [n_heats + 1], [off[n_heats]] ascending within a heat
    int n_heats;
    int heats_fresh;                            // 1: an attachment the log has not seen before
    // the walls' output planes; wall_f null: no walls
    const double *wall_f;                       // [LPVMPC_WALL_F64][B]
    const int32_t *wall_i;                      // [LPVMPC_WALL_I32][B]
    int walls_fresh;
};

struct EventDev {               // passed by value
    int B;
    uint32_t kinds;
    double *carry_f;                            // [LPVMPC_EVENT_CARRY_F64][B]
    int32_t *carry_i;                           // [LPVMPC_EVENT_CARRY_I32][B]
    double *out_f;                              // (no f64 outputs: width 0)
    int32_t *out_i;                             // [LPVMPC_EVENT_OUT_I32][B]
    int32_t *ev_i;                              // [capacity][LPVMPC_EVENT_I32]
    double *ev_f;                               // [capacity][LPVMPC_EVENT_F64]
    long long capacity;                         // slots of the ring; the batch form's max_events
    unsigned long long *total;                  // [1] events since the attach
    int32_t *n_events;                          // [1] events of this tick (null: not wanted)
};

// the heat of each vehicle from the heats' member lists (one thread per member slot; heat_of is set to -1 first)
hipError_t launch_event_heat_of(int B, int n_heats, const int32_t *off, const int32_t *members, int32_t *heat_of, hipStream_t s);
// one tick of the log: the last launch of a race's tick (slots in the ring), and the batch form (slots from index 0)
hipError_t launch_event_tick(const EventDev &e, const EventSrc &s, int t, hipStream_t st);
hipError_t launch_event_step(const EventDev &e, const EventSrc &s, int t, hipStream_t st);

#ifdef __HIPCC__
// exclusive prefix sum of v over the workgroup's threads, and the workgroup's sum.  Every thread calls it; lds holds 64 words
__device__ __forceinline__ int event_block_scan(int v, int *lds, int &sum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    if (w == 0) {
        int y = lane < nw ? lds[lane] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int z = __shfl_up(y, d);
            if (lane >= d) y += z;
        }
        lds[lane] = y;
    }
    __syncthreads();
    const int base = w ? lds[w - 1] : 0;
    sum = lds[nw - 1];
    __syncthreads();                                                        // the next scan writes lds again
    return base + x - v;
}

// The per-vehicle work of a tick for vehicle b: compares before and after and counts the vehicle's events; with kEmit it writes them
// from the tick's index `first` on, in kind order, and updates the carry (all but POSITION / CLASS: event_tick's pass 3) and the
// outputs.  known: the vehicle's count where it is known (pass 2 has pass 1's: a vehicle without events skips the PASS walk), else
// non-zero.  n_tick: the tick's count, total0: the count before the tick.  kLinear: the batch form's slots
template <bool kLinear, bool kEmit>
__device__ __forceinline__ int event_vehicle(const EventDev &e, const EventSrc &s, int t, int b, long long first, long long n_tick,
                                             unsigned long long total0, int known) {
    const size_t B = e.B;
    const double nan = __builtin_nan("");
    int32_t *ci = e.carry_i + b;
    double *cf = e.carry_f + b;
    int cnt = 0;
    auto put = [&](int kind, int other, int a, int bb, double v0, double v1) {
        if (!((e.kinds >> kind) & 1u)) return;
        if constexpr (kEmit) {
            const long long k = first + cnt;
            const bool w = kLinear ? k < e.capacity : k >= n_tick - e.capacity;
            if (w) {
                const long long slot = kLinear ? k : (long long)((total0 + (unsigned long long)k) % (unsigned long long)e.capacity);
                int32_t *pi = e.ev_i + slot * LPVMPC_EVENT_I32;
                double *pf = e.ev_f + slot * LPVMPC_EVENT_F64;
                pi[LPVMPC_EVENT_TICK] = t; pi[LPVMPC_EVENT_KIND] = kind; pi[LPVMPC_EVENT_VEHICLE] = b; pi[LPVMPC_EVENT_OTHER] = other;
                pi[LPVMPC_EVENT_A] = a; pi[LPVMPC_EVENT_B] = bb;
                pf[LPVMPC_EVENT_V0] = v0; pf[LPVMPC_EVENT_V1] = v1;
            }
        }
        ++cnt;
    };
    const int flags = ci[LPVMPC_EVENT_CARRY_FLAGS * B];
    // the race's rows
    const int phase = s.phase[b], lap = s.lap[b];
    if (flags & 1) {
        const int phase0 = ci[LPVMPC_EVENT_CARRY_PHASE * B], lap0 = ci[LPVMPC_EVENT_CARRY_LAP * B];
        if (lap > lap0) {
            double v = nan;
            if (s.lap_value) v = s.lap_value[b];
            else if (lap >= 0 && lap < s.lap_cols) v = (double)s.lap_step[(size_t)b * s.lap_cols + lap];
            put(LPVMPC_EVENT_LAP, -1, lap, phase, v, nan);
        }
        if (phase == 2 && phase0 != 2) put(LPVMPC_EVENT_FINISH, -1, lap, -1, nan, nan);
        if (phase == 3 && phase0 != 3) put(LPVMPC_EVENT_LOST, -1, lap, -1, nan, nan);
    }
    // the heats
    int g = s.heat_f ? s.heat_of[b] : -1;
    if (g >= s.n_heats) g = -1;
    const bool has_h = g >= 0, seen_h = has_h && (flags & 2) && !s.heats_fresh;
    int con = 0, near0 = -1, cstart = -1;
    double cmin = 0.0;
    if (has_h) {
        const int pos = s.heat_i[LPVMPC_HEAT_POSITION * B + b], cls = s.heat_i[LPVMPC_HEAT_CLASS * B + b];
        const int near = s.heat_i[LPVMPC_HEAT_NEAREST * B + b];
        con = s.heat_i[LPVMPC_HEAT_CONTACT * B + b] != 0;
        const double clear = s.heat_f[LPVMPC_HEAT_CLEARANCE * B + b];
        int con0 = 0;
        if (seen_h) {
            con0 = ci[LPVMPC_EVENT_CARRY_CONTACT * B]; near0 = ci[LPVMPC_EVENT_CARRY_NEAREST * B];
            cstart = ci[LPVMPC_EVENT_CARRY_CONTACT_START * B]; cmin = cf[LPVMPC_EVENT_CARRY_MIN_CLEARANCE * B];
            const int pos0 = ci[LPVMPC_EVENT_CARRY_POSITION * B], cls0 = ci[LPVMPC_EVENT_CARRY_CLASS * B];
            // PASS: the members of the heat in ascending vehicle index, with their before / after POSITION and CLASS
            const bool walk = kEmit ? known != 0 : true;
            if (walk && cls0 == 1 && cls == 1 && ((e.kinds >> LPVMPC_EVENT_PASS) & 1u)) {
                const double prog = s.heat_f[LPVMPC_HEAT_PROGRESS * B + b];
                const int k1 = s.off[g + 1];
                for (int k = s.off[g]; k < k1; ++k) {
                    const int j = s.members[k];
                    if (j == b || (unsigned)j >= (unsigned)e.B) continue;
                    const int pj0 = e.carry_i[LPVMPC_EVENT_CARRY_POSITION * B + j], cj0 = e.carry_i[LPVMPC_EVENT_CARRY_CLASS * B + j];
                    const int pj = s.heat_i[LPVMPC_HEAT_POSITION * B + j], cj = s.heat_i[LPVMPC_HEAT_CLASS * B + j];
                    if (cj0 == 1 && cj == 1 && pos0 > pj0 && pos < pj)                  // (PROGRESS is read for a PASS alone)
                        put(LPVMPC_EVENT_PASS, j, pos, pj, prog - s.heat_f[LPVMPC_HEAT_PROGRESS * B + j], nan);
                }
            }
        }
        if (con && !con0) {                                                 // a spell begins (at first sight: without the event)
            if (seen_h) put(LPVMPC_EVENT_CONTACT_BEGIN, near, -1, -1, clear, nan);
            cstart = t; cmin = clear; near0 = near;
        } else if (con) {
            if (clear < cmin) cmin = clear;
            near0 = near;
        } else if (con0) {
            put(LPVMPC_EVENT_CONTACT_END, near0, t - cstart, -1, cmin, nan);
        }
        if (!con) { near0 = -1; cstart = -1; cmin = 0.0; }
    }
    // the walls
    const bool has_w = s.wall_f != nullptr, seen_w = has_w && (flags & 4) && !s.walls_fresh;
    int hit = 0, hstart = -1;
    double wmax = 0.0;
    if (has_w) {
        hit = s.wall_i[LPVMPC_WALL_HIT * B + b] != 0;
        const double imp = s.wall_f[LPVMPC_WALL_IMPULSE * B + b];
        int hit0 = 0;
        if (seen_w) { hit0 = ci[LPVMPC_EVENT_CARRY_HIT * B]; hstart = ci[LPVMPC_EVENT_CARRY_HIT_START * B]; wmax = cf[LPVMPC_EVENT_CARRY_MAX_IMPULSE * B]; }
        if (hit && !hit0) {
            if (seen_w)
                put(LPVMPC_EVENT_WALL_HIT, -1, s.wall_i[LPVMPC_WALL_SIDE * B + b], s.wall_i[LPVMPC_WALL_CORNER * B + b],
                    s.wall_f[LPVMPC_WALL_DEPTH * B + b], imp);
            hstart = t; wmax = imp;
        } else if (hit) {
            if (imp > wmax) wmax = imp;
        } else if (hit0) {
            put(LPVMPC_EVENT_WALL_CLEAR, -1, t - hstart, -1, wmax, nan);
        }
        if (!hit) { hstart = -1; wmax = 0.0; }
    }
    if constexpr (kEmit) {
        const int all = ci[LPVMPC_EVENT_CARRY_COUNT_TOTAL * B] + cnt;
        ci[LPVMPC_EVENT_CARRY_FLAGS * B] = 1 | (has_h ? 2 : 0) | (has_w ? 4 : 0);
        ci[LPVMPC_EVENT_CARRY_PHASE * B] = phase; ci[LPVMPC_EVENT_CARRY_LAP * B] = lap;
        ci[LPVMPC_EVENT_CARRY_CONTACT * B] = con; ci[LPVMPC_EVENT_CARRY_NEAREST * B] = near0; ci[LPVMPC_EVENT_CARRY_CONTACT_START * B] = cstart;
        ci[LPVMPC_EVENT_CARRY_HIT * B] = hit; ci[LPVMPC_EVENT_CARRY_HIT_START * B] = hstart; ci[LPVMPC_EVENT_CARRY_COUNT_TOTAL * B] = all;
        cf[LPVMPC_EVENT_CARRY_MIN_CLEARANCE * B] = cmin; cf[LPVMPC_EVENT_CARRY_MAX_IMPULSE * B] = wmax;
        e.out_i[LPVMPC_EVENT_COUNT * B + b] = cnt; e.out_i[LPVMPC_EVENT_COUNT_TOTAL * B + b] = all;
    }
    return cnt;
}

// one tick of the log, run by ONE workgroup (every thread calls it: it holds the workgroup's barriers)
template <bool kLinear> __device__ __forceinline__ void event_tick(const EventDev &e, const EventSrc &s, int t, int *lds) {
    const int B = e.B, W = blockDim.x, tid = threadIdx.x;
    const size_t Bs = e.B;
    const unsigned long long total0 = *e.total;                             // (written by thread 0 behind the last barrier)
    // pass 1: counts, kept in the COUNT plane for pass 2 (each thread takes the same vehicles in both)
    long long n = 0;
    for (int c0 = 0; c0 < B; c0 += W) {
        const int b = c0 + tid;
        int c = 0;
        if (b < B) { c = event_vehicle<kLinear, false>(e, s, t, b, 0, 0, total0, 1); e.out_i[LPVMPC_EVENT_COUNT * Bs + b] = c; }
        int sum;
        (void)event_block_scan(c, lds, sum);
        n += sum;
    }
    // pass 2: offsets, events, carry.  A vehicle without events skips the walk
    long long base = 0;
    for (int c0 = 0; c0 < B; c0 += W) {
        const int b = c0 + tid;
        const int c = b < B ? e.out_i[LPVMPC_EVENT_COUNT * Bs + b] : 0;
        int sum;
        const int off = event_block_scan(c, lds, sum);
        if (b < B) (void)event_vehicle<kLinear, true>(e, s, t, b, base + off, n, total0, c);
        base += sum;
    }
    __syncthreads();                                                        // no walk of this tick reads a before word any more
    // pass 3: the before words that other vehicles' walks read
    for (int b = tid; b < B; b += W) {
        int g = s.heat_f ? s.heat_of[b] : -1;
        if (g >= s.n_heats) g = -1;
        e.carry_i[LPVMPC_EVENT_CARRY_POSITION * Bs + b] = g >= 0 ? s.heat_i[LPVMPC_HEAT_POSITION * Bs + b] : -1;
        e.carry_i[LPVMPC_EVENT_CARRY_CLASS * Bs + b] = g >= 0 ? s.heat_i[LPVMPC_HEAT_CLASS * Bs + b] : -1;
    }
    if (tid == 0) {
        *e.total = total0 + (unsigned long long)n;
        if (e.n_events) e.n_events[0] = (int32_t)n;
    }
}
#endif  // __HIPCC__

}  // namespace lpvmpc
