// The schedule of the phased k loop of the split contraction (pearson_bf16.hip, SEEKR_GEMM_LOOP=1), as plain C++: the
// kernel's loop IS run_phased_loop() below, instantiated with operations that issue LDS-DMA pieces, ds_reads, waits,
// barriers and MFMAs; tests/phased_schedule_model.cpp instantiates the same function with operations that only record,
// for both wave groups, and checks the ordering rules on the recorded program.  Nothing here touches the GPU.
//
// Units.  A k tile (64 KiB of LDS: 256 A rows and 256 B rows of one 128-byte line) is consumed in kPhases = 4 phases of
// 24 MFMAs per wave: phase h multiplies the wave's A row tiles 2h and 2h + 1 by all four of its B row tiles.  B is read
// once per k tile (phase 0) and held; A is read by quarters.  What phase h READS is "unit" 4 t + h of k tile t:
//     unit 4 t     : the B tile and the A rows of row tiles 0-1 of both wave rows   5 LDS-DMA pieces per wave
//     unit 4 t + h : the A rows of row tiles 2h, 2h + 1 of both wave rows           1 piece per wave
// The two 64 KiB stages form a ring of kRing = 8 unit buffers; unit u lives in buffer u % 8 (stage (u / 4) % 2, the
// addresses the present loop uses).  Every wave issues the same number of pieces of every unit, so one count holds for
// all of them.
//
// Order (cdna_hip_programming.md, the 256 x 256 8-phase template).  The waves of wave row 1 ("behind") take one barrier
// more in front of the loop and the others one more after it: while one group is inside an MFMA cluster the other
// issues its reads and DMA.  Number the intervals between barriers I(0), I(1), ... from the prologue's barrier; phase p
// of the leading group reads in I(2p) and multiplies in I(2p + 1), the group behind in I(2p + 1) and I(2p + 2).
//   RAW: unit p + 1 is waited for (counted vmcnt, by every wave, for its own pieces) in the READ part of phase p, in front
//        of that phase's first barrier, and read in phase p + 1: the latest wait is in I(2p + 1), the earliest read in
//        I(2p + 2) — one barrier both groups have passed lies between.
//   WAR: the reads of unit p - 2 are complete (lgkmcnt(0)) in I(2p - 3) / I(2p - 2); its buffer is restaged with unit
//        p + 6 in the read part of phase p, I(2p) / I(2p + 1): after a barrier that follows BOTH groups' last read.
//        kAhead = 6 is the largest depth for which that holds (unit p + 7 would overwrite what the group behind may
//        still be reading in I(2p)).
//   N:   pieces are retired in the order issued, so the wait for unit p + 1 leaves exactly the pieces of the units
//        issued after it: p + 2 .. min(p + 6, last unit).  In the steady state that is 9, 9, 13, 9 for phases 0-3 — never
//        0: five units (1.25 k tiles) stay in flight across every barrier.
//   Barriers: 2 per phase + 1 prologue + 1 stagger for either group, on every path (kt = 1, odd, even, tail).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SKR_SCHED_FN __host__ __device__ __forceinline__
#else
#define SKR_SCHED_FN inline
#endif

namespace skr_phased {

template <int N>
struct Int {
    static constexpr int value = N;
};

constexpr int kPhases = 4;                 // per k tile
constexpr int kRing = 2 * kPhases;         // unit buffers in the two stages
constexpr int kAhead = 6;                  // phase p issues unit p + kAhead
constexpr int kPiecesB = 4, kPiecesA = 1;  // per wave: B pieces of a k tile (all in its unit 0), A pieces per unit

constexpr int pieces(int unit) { return unit % kPhases == 0 ? kPiecesB + kPiecesA : kPiecesA; }

// units after this one when phase `ph` of a k tile with `tiles_after` more tiles behind it runs
constexpr int units_after(int ph, int tiles_after) { return kPhases * tiles_after + (kPhases - 1 - ph); }

// does phase `ph` issue unit (this + kAhead)?  tiles_after >= 2 stands for the steady state
constexpr bool issues(int ph, int tiles_after) { return units_after(ph, tiles_after) >= kAhead; }

// N of the counted wait in phase `ph`: pieces of the units this + 2 .. this + min(kAhead, units after); -1: nothing left
// to wait for (the last phase)
constexpr int wait_n(int ph, int tiles_after) {
    const int after = units_after(ph, tiles_after);
    if (after < 1) return -1;
    const int last = after < kAhead ? after : kAhead;
    int n = 0;
    for (int d = 2; d <= last; d++) n += pieces(ph + d);
    return n;
}

// prologue: units 0 .. prologue_units - 1 are issued, unit 0 is waited for
constexpr int prologue_units(bool one_tile) { return one_tile ? kPhases : kAhead; }
constexpr int prologue_wait(bool one_tile) {
    int n = 0;
    for (int u = 1; u < prologue_units(one_tile); u++) n += pieces(u);
    return n;
}

// One phase.  Ops: issue(tile, Int<phase>) — this wave's pieces of that unit into its buffer; read(tile, Int<phase>) —
// the ds_reads of the unit; wait_vm(Int<N>); barrier(); wait_lgkm(); mfma(Int<phase>).
template <int PH, int TILES_AFTER, class Ops>
SKR_SCHED_FN void phase(Ops& ops, int64_t t) {
    ops.read(t, Int<PH>{});
    if constexpr (issues(PH, TILES_AFTER)) ops.issue(t + (PH + kAhead) / kPhases, Int<(PH + kAhead) % kPhases>{});
    if constexpr (wait_n(PH, TILES_AFTER) >= 0) ops.wait_vm(Int<wait_n(PH, TILES_AFTER)>{});
    ops.barrier();
    ops.wait_lgkm();
    ops.mfma(Int<PH>{});
    ops.barrier();
}

template <int TILES_AFTER, class Ops>
SKR_SCHED_FN void tile(Ops& ops, int64_t t) {
    phase<0, TILES_AFTER>(ops, t);
    phase<1, TILES_AFTER>(ops, t);
    phase<2, TILES_AFTER>(ops, t);
    phase<3, TILES_AFTER>(ops, t);
}

// The whole k loop of one output tile for one wave.  `behind`: the wave belongs to the group that runs one barrier late
// (wave-uniform).  kt >= 1.  On entry no DMA of this wave into the stages is pending and every wave of the workgroup has
// passed a barrier after its last read of them; on exit both hold again.
template <class Ops>
SKR_SCHED_FN void run_phased_loop(Ops& ops, int64_t kt, bool behind) {
    if (kt == 1) {
        ops.issue(0, Int<0>{});
        ops.issue(0, Int<1>{});
        ops.issue(0, Int<2>{});
        ops.issue(0, Int<3>{});
        ops.wait_vm(Int<prologue_wait(true)>{});
    } else {
        ops.issue(0, Int<0>{});
        ops.issue(0, Int<1>{});
        ops.issue(0, Int<2>{});
        ops.issue(0, Int<3>{});
        ops.issue(1, Int<0>{});
        ops.issue(1, Int<1>{});
        static_assert(kAhead == kPhases + 2, "the prologue above issues kAhead units");
        ops.wait_vm(Int<prologue_wait(false)>{});
    }
    ops.barrier();
    if (behind) ops.barrier();
    int64_t t = 0;
    for (; t + 2 < kt; t++) tile<2>(ops, t);
    if (t + 1 < kt) {
        tile<1>(ops, t);
        t++;
    }
    tile<0>(ops, t);
    if (!behind) ops.barrier();
}

}  // namespace skr_phased
