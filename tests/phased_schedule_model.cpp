// Host model of the phased k loop of the split contraction (seekr_amd/csrc/gemm_phased_schedule.hpp, SEEKR_GEMM_LOOP=1).
// The kernel's loop is run_phased_loop() instantiated with GPU operations; here the SAME function runs with operations
// that only record, once per wave group, and the recorded programs are checked against the ordering rules of LDS-DMA
// staging (cdna_hip_programming.md, the 256 x 256 8-phase template):
//   - both groups take the same number of barriers on every path (a difference hangs the workgroup);
//   - every counted wait retires exactly the pieces of one unit and leaves exactly N pieces outstanding;
//   - a unit is read only after EVERY wave's wait for it and a barrier both groups have passed since;
//   - a buffer is restaged only after both groups' reads of its previous unit are complete (lgkmcnt(0)) and a barrier
//     both groups have passed since;
//   - the groups run one barrier apart: one reads while the other multiplies.
// Built by tests/test_phased_schedule.py with the host compiler and -fsanitize=address,undefined; no GPU involved.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#include "../seekr_amd/csrc/gemm_phased_schedule.hpp"

namespace {

using skr_phased::Int;

// the geometry, restated from the kernel and not taken from the header under test: 8 waves; an LDS-DMA piece is 8 rows
// of one 128-byte line; the B tile has 256 rows; a unit holds two 16-row A tiles of each of the two wave rows
constexpr int kWaves = 8, kRowsPerPiece = 8, kUnitsPerTile = 4, kBuffers = 8;
constexpr int kBPiecesPerWave = 256 / kRowsPerPiece / kWaves;          // 4
constexpr int kAPiecesPerWave = 2 * 16 * 2 / kRowsPerPiece / kWaves;  // 1
int model_pieces(int64_t unit) { return unit % kUnitsPerTile == 0 ? kBPiecesPerWave + kAPiecesPerWave : kAPiecesPerWave; }

struct Event {
    enum Kind { ISSUE, READ, WAIT_VM, WAIT_LGKM, MFMA } kind;
    int64_t unit;  // ISSUE / READ: the unit; MFMA: the phase within the tile
    int n;         // WAIT_VM: N
    int interval;  // barriers this wave has passed
};

struct Recorder {
    std::vector<Event> ev;
    int barriers = 0;
    template <int U>
    void issue(int64_t tile, Int<U>) { ev.push_back({Event::ISSUE, tile * kUnitsPerTile + U, 0, barriers}); }
    template <int U>
    void read(int64_t tile, Int<U>) { ev.push_back({Event::READ, tile * kUnitsPerTile + U, 0, barriers}); }
    template <int N>
    void wait_vm(Int<N>) { ev.push_back({Event::WAIT_VM, -1, N, barriers}); }
    void wait_lgkm() { ev.push_back({Event::WAIT_LGKM, -1, 0, barriers}); }
    template <int U>
    void mfma(Int<U>) { ev.push_back({Event::MFMA, U, 0, barriers}); }
    void barrier() { barriers++; }
};

int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            failures++;                                   \
            std::fprintf(stderr, "FAIL %s: ", #cond);     \
            std::fprintf(stderr, __VA_ARGS__);            \
            std::fprintf(stderr, "\n");                   \
        }                                                 \
    } while (0)

struct Facts {  // what one group's program establishes, per unit
    std::vector<int> issued, retired, read_at, read_done, mfma_at;
};

Facts walk(const Recorder& r, int64_t kt, int group, bool* steady_zero_wait) {
    const int64_t units = kt * kUnitsPerTile;
    Facts f;
    f.issued.assign(units, -1);
    f.retired.assign(units, -1);
    f.read_at.assign(units, -1);
    f.read_done.assign(units, -1);
    f.mfma_at.assign(units, -1);
    std::deque<int64_t> vm;  // one entry per outstanding piece of this wave, oldest first: the in-order counter
    int64_t next_issue = 0, next_retire = 0, next_read = 0, next_mfma = 0, pending_read = -1;
    for (const Event& e : r.ev) {
        switch (e.kind) {
            case Event::ISSUE:
                CHECK(e.unit == next_issue && e.unit < units, "kt %lld group %d: unit %lld issued out of order or past the end", (long long)kt, group, (long long)e.unit);
                if (e.unit >= 0 && e.unit < units) f.issued[e.unit] = e.interval;
                for (int p = 0; p < model_pieces(e.unit); p++) vm.push_back(e.unit);
                next_issue = e.unit + 1;
                break;
            case Event::WAIT_VM: {
                // the wait is for the oldest unit not yet retired: it must retire exactly that unit's pieces
                CHECK(next_retire < next_issue, "kt %lld group %d: vmcnt(%d) with nothing to wait for", (long long)kt, group, e.n);
                int popped = 0;
                bool only_target = true;
                while ((int)vm.size() > e.n) {
                    only_target = only_target && vm.front() == next_retire;
                    vm.pop_front();
                    popped++;
                }
                CHECK(only_target && popped == model_pieces(next_retire) && (int)vm.size() == e.n,
                      "kt %lld group %d: vmcnt(%d) for unit %lld retires %d pieces (want %d, of that unit only), leaves %d",
                      (long long)kt, group, e.n, (long long)next_retire, popped, model_pieces(next_retire), (int)vm.size());
                CHECK(vm.empty() || vm.front() == next_retire + 1, "kt %lld group %d: unit %lld only partly retired", (long long)kt, group, (long long)next_retire);
                if (next_retire < units) f.retired[next_retire] = e.interval;
                // steady state: three or more tiles, the wait sits in a tile with two more behind it
                if (e.n == 0 && next_retire + 1 + 2 * kUnitsPerTile < units) *steady_zero_wait = true;
                next_retire++;
                break;
            }
            case Event::READ:
                CHECK(e.unit == next_read && pending_read < 0, "kt %lld group %d: unit %lld read out of order", (long long)kt, group, (long long)e.unit);
                if (e.unit >= 0 && e.unit < units) f.read_at[e.unit] = e.interval;
                pending_read = e.unit;
                next_read = e.unit + 1;
                break;
            case Event::WAIT_LGKM:
                CHECK(pending_read >= 0, "kt %lld group %d: lgkmcnt wait without a read", (long long)kt, group);
                if (pending_read >= 0 && pending_read < units) f.read_done[pending_read] = e.interval;
                break;
            case Event::MFMA:
                CHECK(pending_read == next_mfma && e.unit == next_mfma % kUnitsPerTile && f.read_done[next_mfma] >= 0,
                      "kt %lld group %d: MFMA cluster %lld without its completed reads", (long long)kt, group, (long long)next_mfma);
                CHECK(e.interval == f.read_at[next_mfma] + 1, "kt %lld group %d: MFMA cluster %lld is not one barrier after its reads", (long long)kt, group, (long long)next_mfma);
                f.mfma_at[next_mfma] = e.interval;
                pending_read = -1;
                next_mfma++;
                break;
        }
    }
    CHECK(next_issue == units && next_retire == units && next_read == units && next_mfma == units && vm.empty(),
          "kt %lld group %d: %lld issued, %lld retired, %lld read, %lld multiplied of %lld units, %d pieces pending at the end",
          (long long)kt, group, (long long)next_issue, (long long)next_retire, (long long)next_read, (long long)next_mfma, (long long)units, (int)vm.size());
    return f;
}

void check(int64_t kt) {
    Recorder rec[2];
    skr_phased::run_phased_loop(rec[0], kt, false);
    skr_phased::run_phased_loop(rec[1], kt, true);
    const int64_t units = kt * kUnitsPerTile;
    CHECK(rec[0].barriers == rec[1].barriers, "kt %lld: %d barriers in the leading group, %d in the one behind", (long long)kt, rec[0].barriers, rec[1].barriers);
    CHECK(rec[0].barriers == 2 * units + 2, "kt %lld: %d barriers, want two per phase, the prologue's and the stagger's", (long long)kt, rec[0].barriers);
    bool steady_zero_wait = false;
    const Facts f[2] = {walk(rec[0], kt, 0, &steady_zero_wait), walk(rec[1], kt, 1, &steady_zero_wait)};
    CHECK(!steady_zero_wait, "kt %lld: vmcnt(0) in the steady state", (long long)kt);
    for (int64_t u = 0; u < units; u++) {
        for (int g = 0; g < 2; g++)
            for (int h = 0; h < 2; h++) {
                // RAW: group h's waves have waited for their pieces of u, and a barrier passed by both lies before g's read
                CHECK(f[h].retired[u] >= 0 && f[h].retired[u] + 1 <= f[g].read_at[u],
                      "kt %lld: group %d reads unit %lld in interval %d, group %d waits for it in interval %d", (long long)kt, g, (long long)u, f[g].read_at[u], h, f[h].retired[u]);
                // WAR: the previous unit of the buffer has been read completely by h, with a barrier before g restages it
                if (u >= kBuffers)
                    CHECK(f[h].read_done[u - kBuffers] >= 0 && f[h].read_done[u - kBuffers] + 1 <= f[g].issued[u],
                          "kt %lld: group %d restages buffer %lld with unit %lld in interval %d, group %d finishes reading it in interval %d",
                          (long long)kt, g, (long long)(u % kBuffers), (long long)u, f[g].issued[u], h, f[h].read_done[u - kBuffers]);
            }
        // the stagger: the group behind reads while the leading one multiplies, and multiplies one barrier later
        CHECK(f[1].read_at[u] == f[0].mfma_at[u] && f[1].mfma_at[u] == f[0].mfma_at[u] + 1, "kt %lld: the groups are not one barrier apart at unit %lld", (long long)kt, (long long)u);
    }
}

}  // namespace

int main() {
    const long long kts[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 32, 33, 128};
    for (long long kt : kts) check(kt);
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("phased schedule ok: %d loop lengths, both groups\n", (int)(sizeof(kts) / sizeof(kts[0])));
    return 0;
}
