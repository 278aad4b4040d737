// race_attach.hpp -- the host scaffold of what attaches to a running race: the heats, the interactions, the contact model, the walls
// and the event log (heats_api.hip, interactions_api.hip, contact_api.hip, walls_api.hip, events_api.hip) and race_api.hip, which owns
// the five slots.  Host code only: no kernel translation unit includes it.  A layer supplies its configuration check, its blank-output rule, the fields of its
// kernel argument and its launch; the allocation, the four planes, the entry points' prologues, the whole-or-nothing install, the read
// entry point and the detach chain are here ("Race attachments").
#pragma once
#include "lpvmpc_handle.hpp"

#pragma GCC visibility push(hidden)   // nothing here is part of the library's ABI

// an int-returning step of an entry point: a refusal or failure ends the entry point with its code
#define RC_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

struct HeatsBinding;         // heats_host.hpp
struct InterBinding;         // interactions_host.hpp
struct ContactBinding;       // contact_host.hpp
struct WallBinding;          // walls_host.hpp
struct EventBinding;         // events_host.hpp

// race_api.hip: what an attachment needs of the running race: its shape, the state a tick reads and writes, the plant side whose live
// table the layers read and rewrite, and the five slots that own the bindings, with the serials of the two slots that the event log
// observes (false: the handle owns no race)
struct RaceAttachView {
    int B = 0, laps = 0;
    double hw = 0, slack = 0;
    double *plant = nullptr;
    const int32_t *nstep = nullptr, *phase = nullptr;
    PlantSide *side = nullptr;
    std::unique_ptr<HeatsBinding> *heats = nullptr;
    std::unique_ptr<InterBinding> *inter = nullptr;
    std::unique_ptr<ContactBinding> *contact = nullptr;
    std::unique_ptr<WallBinding> *walls = nullptr;
    std::unique_ptr<EventBinding> *events = nullptr;
    uint32_t *heats_serial = nullptr, *walls_serial = nullptr;                  // bumped wherever that slot's binding is installed or detached
};
LPVMPC_HIDDEN bool lpvmpc_race_attach_view(lpvmpc_handle *h, RaceAttachView &v);

// race_api.hip: detaches one layer of h's race with the layers that read it, readers first: the heats take the interactions with them
// (their binding reads the heats' lists and extents), the interactions the contact model (its kernel argument is a copy of theirs);
// the walls stand alone, and so does the event log (no layer reads it and it reads no binding).  Each binding goes once no tick in flight reads it, and the interactions put the base mu words back into the
// live plant table.  No race, or nothing attached: nothing to do.  _readers: the readers alone, ahead of a layer's replacement
enum RaceLayer { RACE_HEATS, RACE_INTERACTIONS, RACE_CONTACT, RACE_WALLS, RACE_EVENTS };
LPVMPC_HIDDEN int lpvmpc_race_detach(lpvmpc_handle *h, RaceLayer layer);
LPVMPC_HIDDEN int lpvmpc_race_detach_readers(lpvmpc_handle *h, RaceLayer layer);

// The prologue of an entry point that acts on the race's attachments: the view, or the refusal, then the device and the stream
struct RaceAttach {
    RaceAttachView v;
    hipStream_t st = nullptr;
    int begin(lpvmpc_handle *h, const char *who) {
        if (!h || !lpvmpc_race_attach_view(h, v)) return fail(h, LPVMPC_E_ARG, "%s: call lpvmpc_race_init first", who);
        HIP_TRY(h, hipSetDevice(h->cfg.device));
        st = h->stream;
        return LPVMPC_OK;
    }
};

// The prologue of a _step_batch entry point.  true: the call ends here with rc (B == 0: nothing to do; no handle; a busy handle)
inline bool lpvmpc_batch_done(lpvmpc_handle *h, int B, const char *who, int &rc) {
    if (h && B == 0) rc = LPVMPC_OK;
    else if (!h) rc = fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    else if (busy(h)) rc = fail(h, LPVMPC_E_ARG, "%s: this handle runs a fleet, cascade or race; use another handle for batch calls", who);
    else return false;
    return true;
}

// Allocations of one entry point out of one arena: stops at the first failed hipMalloc and remembers its size; an empty array takes
// 8 bytes, so that every pointer is one hipFree can take and a kernel argument is never null by accident
struct DevTake {
    DevArena &mem;
    hipError_t err = hipSuccess;
    size_t want = 0;
    template <class T> void operator()(T *&p, size_t bytes) {
        if (err == hipSuccess) { want = bytes; err = mem.alloc(p, bytes ? bytes : 8); }
    }
    // LPVMPC_OK, or LPVMPC_E_NOMEM in the words of an attach (sized) or of a batch call
    int check(lpvmpc_handle *h, const char *who, bool sized) const {
        if (err == hipSuccess) return LPVMPC_OK;
        if (sized) return fail(h, LPVMPC_E_NOMEM, "%s: hipMalloc of %zu B failed: %s", who, want, hipGetErrorString(err));
        return fail(h, LPVMPC_E_NOMEM, "%s: hipMalloc failed: %s", who, hipGetErrorString(err));
    }
};

// The four planes of a layer, [W][B] each: the carried state and the outputs, in doubles and in 32-bit integers.  The pointers are the
// fields of the layer's kernel argument (every one names them carry_f, carry_i, out_f, out_i); every byte count of a plane is made here
struct Planes {
    size_t B;
    int carry_f64, carry_i32, f64, i32;                                         // the widths W
    double *&carry_f;
    int32_t *&carry_i;
    double *&out_f;
    int32_t *&out_i;
    size_t carry_f_bytes() const { return B * carry_f64 * 8; }
    size_t carry_i_bytes() const { return B * carry_i32 * 4; }
    size_t out_f_bytes() const { return B * f64 * 8; }
    size_t out_i_bytes() const { return B * i32 * 4; }
    void alloc(DevTake &take) const { take(carry_f, carry_f_bytes()); take(carry_i, carry_i_bytes()); take(out_f, out_f_bytes()); take(out_i, out_i_bytes()); }
    // a fresh carry: zeros, the integers from ci [carry_i32][B] where a layer's rule sets some (null: zeros too)
    int blank_carry(lpvmpc_handle *h, hipStream_t st, const int32_t *ci) const {
        HIP_TRY(h, hipMemsetAsync(carry_f, 0, carry_f_bytes(), st));
        if (ci) H2D(carry_i, ci, carry_i_bytes());
        else HIP_TRY(h, hipMemsetAsync(carry_i, 0, carry_i_bytes(), st));
        return LPVMPC_OK;
    }
    // what a vehicle reads before its first tick, by the layer's rule; the vectors outlive the copies
    int blank_out(lpvmpc_handle *h, hipStream_t st, const std::vector<double> &f, const std::vector<int32_t> &i) const {
        H2D(out_f, f.data(), out_f_bytes());
        H2D(out_i, i.data(), out_i_bytes());
        return LPVMPC_OK;
    }
    int read(lpvmpc_handle *h, hipStream_t st, double *f, int32_t *i) const {  // each may be null
        if (f) D2H(f, out_f, out_f_bytes());
        if (i) D2H(i, out_i, out_i_bytes());
        return LPVMPC_OK;
    }
    // the batch form: the caller's carry in, and carry and outputs back
    int carry_in(lpvmpc_handle *h, hipStream_t st, const double *cf, const int32_t *ci) const {
        H2D(carry_f, cf, carry_f_bytes());
        H2D(carry_i, ci, carry_i_bytes());
        return LPVMPC_OK;
    }
    int copy_out(lpvmpc_handle *h, hipStream_t st, double *cf, int32_t *ci, double *f, int32_t *i) const {
        D2H(cf, carry_f, carry_f_bytes());
        D2H(ci, carry_i, carry_i_bytes());
        return read(h, st, f, i);
    }
};
template <class Dev> Planes lpvmpc_planes(Dev &d, size_t B, int carry_f64, int carry_i32, int f64, int i32) {
    return Planes{B, carry_f64, carry_i32, f64, i32, d.carry_f, d.carry_i, d.out_f, d.out_i};
}

// Runs the copies and launches of an entry point to their end on st.  The trailing synchronisation is made whether they succeeded or
// not: the host vectors they read outlive the copies, and nothing in flight reads a device buffer that the caller frees next
template <class Run> int lpvmpc_run_synced(lpvmpc_handle *h, hipStream_t st, Run run) {
    auto whole = [&]() -> int {
        RC_TRY(run());
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    const int rc = whole();
    if (rc) (void)hipStreamSynchronize(st);
    return rc;
}

// The whole-or-nothing install of a binding built in a local: a failed upload leaves the slot as it was, and the binding that the slot
// held is freed only after the synchronisation (no tick in flight reads it).  serial: the slot's serial, where the event log observes
// the slot (RaceAttachView)
template <class Q, class Run>
int lpvmpc_race_install(lpvmpc_handle *h, hipStream_t st, std::unique_ptr<Q> &slot, std::unique_ptr<Q> &q, Run run, uint32_t *serial = nullptr) {
    RC_TRY(lpvmpc_run_synced(h, st, run));
    slot = std::move(q);
    if (serial) ++*serial;
    return LPVMPC_OK;
}

// The read entry point of a layer: its output planes to f64 / i32 (each may be null), then what `more` copies besides (the heats' line
// tables).  missing: the refusal, after "who: ", when nothing is attached
template <class Q, class More>
int lpvmpc_race_read_planes(lpvmpc_handle *h, const char *who, std::unique_ptr<Q> *RaceAttachView::*slot, const char *missing, Planes (*planes)(Q &),
                            double *f64, int32_t *i32, More more) {
    RaceAttach a;
    RC_TRY(a.begin(h, who));
    Q *q = (a.v.*slot)->get();
    if (!q) return fail(h, LPVMPC_E_ARG, "%s: %s", who, missing);
    hipStream_t st = a.st;
    RC_TRY(planes(*q).read(h, st, f64, i32));
    RC_TRY(more(*q, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}
template <class Q>
int lpvmpc_race_read_planes(lpvmpc_handle *h, const char *who, std::unique_ptr<Q> *RaceAttachView::*slot, const char *missing, Planes (*planes)(Q &),
                            double *f64, int32_t *i32) {
    return lpvmpc_race_read_planes(h, who, slot, missing, planes, f64, i32, [](Q &, hipStream_t) { return LPVMPC_OK; });
}

// The heats' member lists on the device, as every form of the three heat-bound layers uploads them: off [n_heats + 1], members
struct HeatLists {
    int32_t *off = nullptr, *members = nullptr;
    void alloc(DevTake &take, const std::vector<int32_t> &o, const std::vector<int32_t> &m) { take(off, o.size() * 4); take(members, m.size() * 4); }
    int upload(lpvmpc_handle *h, hipStream_t st, const std::vector<int32_t> &o, const std::vector<int32_t> &m) const {
        H2D(off, o.data(), o.size() * 4);
        if (!m.empty()) H2D(members, m.data(), m.size() * 4);
        return LPVMPC_OK;
    }
};

// The heat of each vehicle [B] (-1: none), from the heats' lists as they were uploaded (synchronises st twice: the second copy's size
// is in the first)
inline int lpvmpc_heat_of(lpvmpc_handle *h, hipStream_t st, int n_heats, const int32_t *d_off, const int32_t *d_members, size_t B,
                          std::vector<int32_t> &heat_of) {
    std::vector<int32_t> off((size_t)n_heats + 1), members;
    D2H(off.data(), d_off, off.size() * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    members.resize((size_t)off[n_heats]);
    if (!members.empty()) D2H(members.data(), d_members, members.size() * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    heat_of.assign(B, -1);
    for (int g = 0; g < n_heats; ++g)
        for (int k = off[g]; k < off[g + 1]; ++k) heat_of[(size_t)members[k]] = g;
    return LPVMPC_OK;
}
#pragma GCC visibility pop
