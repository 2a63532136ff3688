// tests/cpu/hip_lanes/hip_lanes_waves.h -- TEST INFRASTRUCTURE, NOT HIP: the wavefront model of the stand-in.  hip/hip_runtime.h
// includes it when the lane program defines HIP_LANES_WAVES in front of the kernel file's text; then hipLaunchKernelGGL runs here.
//
// Execution.  One workgroup at a time.  Every lane of the workgroup is a ucontext fiber on a stack of its own; a lane runs until it
// reaches a collective (a shuffle, a ballot, readlane, DPP, ...), a barrier (__syncthreads) or its end.  Lanes are grouped into
// wavefronts of 64 by their flat thread number.  A collective completes when every lane of the wavefront that has not returned
// waits at it; a barrier completes when every lane of the workgroup that has not returned waits at it.  Between two barriers the
// wavefronts run one after the other in the order hip_lanes::order says, each until all its lanes wait at the barrier or have
// returned; between two collectives the lanes of a wavefront run one after the other in that order; the workgroups of a launch run
// in that order as well.  (The shuffled order draws a new permutation every time.)
//
// Reports.  Each ends the program with an exit code of its own and "hip_lanes: <what> at <file>:<line>" on stderr:
//   70  lanes of one wavefront wait at collectives of different call sites
//   71  a wavefront waits partly at a collective and partly at a barrier
//   72  lanes of one workgroup wait at barriers of different call sites
//   73  a shuffle, readlane or DPP read whose source lane has returned, does not exist or is out of range
//   74  a workgroup in which nothing can run and not everything has ended.  With the rules above this cannot come about -- a lane
//       that can run is run, and lanes that wait are either released or reported by 70 .. 72 -- so it is a check of the scheduler
//       itself, kept for the day a kernel's lane program is allowed a divergence at some call site; no wrong kernel reaches it
//   75  the model itself cannot go on (no symbol table to find a kernel's LDS in, no memory for the stacks)
// The site is the line of the collective's call, taken with __builtin_FILE() / __builtin_LINE() as default arguments; for the
// operations of wave_ops.h that is the line in wave_ops.h.
//
// LDS.  __shared__ is `static`, so the host sanitizers put their red zones round every array.  Before each workgroup every
// writable function-local static of the launched kernel function (found by its name in the program's own symbol table) is filled
// with bytes drawn from the seed, the lane order and the workgroup's number: nothing is left from the workgroup before, and a read
// of LDS nobody wrote gives other bytes in every order.  A __shared__ array declared in a __device__ function a kernel calls is not
// found by this and keeps what the last workgroup left.
//
// What this cannot see: timing; the memory model between workgroups (they never overlap here); races between lanes of a
// wavefront that the hardware's lockstep decides (here the lanes between two collectives run one after the other, in three
// orders -- a kernel that needs lockstep gives other bytes in one of them, but which lane the hardware lets win is not modelled).
#pragma once
#include <elf.h>
#include <fcntl.h>
#include <link.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <ucontext.h>
#include <unistd.h>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
extern "C" void __sanitizer_start_switch_fiber(void** fake_stack_save, const void* bottom, size_t size);
extern "C" void __sanitizer_finish_switch_fiber(void* fake_stack_save, const void** bottom_old, size_t* size_old);
#define HIP_LANES_NO_ASAN __attribute__((no_sanitize_address))
#else
#define HIP_LANES_NO_ASAN
#endif

namespace hip_lanes {

enum { EXIT_COLLECTIVE_SITES = 70, EXIT_COLLECTIVE_AND_BARRIER = 71, EXIT_BARRIER_SITES = 72, EXIT_SOURCE_LANE = 73, EXIT_STUCK = 74,
       EXIT_MODEL = 75 };
enum { READY = 0, AT_COLLECTIVE = 1, AT_BARRIER = 2, DONE = 3 };
constexpr size_t kStackBytes = 256 * 1024;

struct LaneCtx {
    ucontext_t ctx;
    int state;
    unsigned flat;              // flat thread number in the workgroup
    dim3 tid;
    const char* file;           // the site it waits at
    int line;
    uint64_t posted;            // what it brought to the collective
};

struct WaveSnap {
    uint64_t vals[64];
    uint64_t present;           // lanes that took part
};

struct GroupRun {
    std::vector<LaneCtx> lanes;
    std::vector<WaveSnap> waves;
    LaneCtx* current = nullptr;
    ucontext_t sched;
    char* stacks = nullptr;
    size_t stacks_lanes = 0;
    const void* sched_bottom = nullptr;
    size_t sched_size = 0;
    void (*body)(void*) = nullptr;
    void* body_arg = nullptr;
    uint64_t rng = 0;
};
inline GroupRun g_run;

[[noreturn]] inline void report(int code, const char* what, const char* file, int line) {
    fprintf(stderr, "hip_lanes: %s at %s:%d (workgroup %u,%u,%u)\n", what, file ? file : "?", line, blockIdx.x, blockIdx.y, blockIdx.z);
    fflush(stderr);
    _exit(code);
}

// ---- switching
inline void to_lane(LaneCtx& l) {
    g_run.current = &l;
    threadIdx = l.tid;
#if defined(__SANITIZE_ADDRESS__)
    void* fake = nullptr;
    __sanitizer_start_switch_fiber(&fake, g_run.stacks + (size_t)l.flat * kStackBytes, kStackBytes);
#endif
    swapcontext(&g_run.sched, &l.ctx);
#if defined(__SANITIZE_ADDRESS__)
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
    g_run.current = nullptr;
}

inline void to_scheduler(bool dying) {
    LaneCtx& l = *g_run.current;
#if defined(__SANITIZE_ADDRESS__)
    void* fake = nullptr;
    __sanitizer_start_switch_fiber(dying ? nullptr : &fake, g_run.sched_bottom, g_run.sched_size);
#endif
    swapcontext(&l.ctx, &g_run.sched);
#if defined(__SANITIZE_ADDRESS__)
    __sanitizer_finish_switch_fiber(fake, &g_run.sched_bottom, &g_run.sched_size);
#endif
    (void)dying;
}

inline void lane_entry() {
#if defined(__SANITIZE_ADDRESS__)
    __sanitizer_finish_switch_fiber(nullptr, &g_run.sched_bottom, &g_run.sched_size);
#endif
    g_run.body(g_run.body_arg);
    g_run.current->state = DONE;
    to_scheduler(true);
    abort();        // (a lane that has ended is not resumed)
}

// ---- what a lane calls
inline unsigned lane_id() { return g_run.current->flat & 63u; }

inline const WaveSnap& collective(uint64_t v, const char* file, int line) {
    LaneCtx& l = *g_run.current;
    l.posted = v;
    l.file = file;
    l.line = line;
    l.state = AT_COLLECTIVE;
    to_scheduler(false);
    return g_run.waves[l.flat >> 6];
}

inline void barrier(const char* file, int line) {
    LaneCtx& l = *g_run.current;
    l.file = file;
    l.line = line;
    l.state = AT_BARRIER;
    to_scheduler(false);
}

inline uint64_t from_lane(const WaveSnap& w, int src, const char* what, const char* file, int line) {
    if (src < 0 || src > 63 || !((w.present >> src) & 1ull)) {
        char text[160];
        snprintf(text, sizeof text, "%s by lane %u from lane %d, which has returned, does not exist or is out of range", what, lane_id(), src);
        report(EXIT_SOURCE_LANE, text, file, line);
    }
    return w.vals[src];
}

// ---- the scheduler
inline void make_order(std::vector<unsigned>& v, unsigned n) {
    v.resize(n);
    for (unsigned i = 0; i < n; i++) v[i] = order == DESCENDING ? n - 1 - i : i;
    if (order == SHUFFLED)
        for (unsigned i = n; i > 1; i--) std::swap(v[i - 1], v[next_random(g_run.rng) % i]);
}

inline void run_wave(unsigned w, unsigned n_lanes) {
    const unsigned lo = w * 64, hi = lo + 64 < n_lanes ? lo + 64 : n_lanes;
    std::vector<unsigned> ord;
    for (;;) {
        make_order(ord, hi - lo);
        for (unsigned k : ord)
            if (g_run.lanes[lo + k].state == READY) to_lane(g_run.lanes[lo + k]);
        const LaneCtx* first = nullptr;
        const LaneCtx* at_barrier = nullptr;
        for (unsigned i = lo; i < hi; i++) {
            const LaneCtx& l = g_run.lanes[i];
            if (l.state == AT_BARRIER) at_barrier = &l;
            if (l.state != AT_COLLECTIVE) continue;
            if (!first) first = &l;
            else if (first->line != l.line || strcmp(first->file, l.file)) {
                char text[200];
                snprintf(text, sizeof text, "lanes %u and %u of wavefront %u wait at collectives of different call sites, the other %s:%d,",
                         first->flat & 63u, l.flat & 63u, w, first->file, first->line);
                report(EXIT_COLLECTIVE_SITES, text, l.file, l.line);
            }
        }
        if (!first) return;
        if (at_barrier) {
            char text[200];
            snprintf(text, sizeof text, "wavefront %u waits partly at a barrier (lane %u, %s:%d) and partly at a collective (lane %u)", w,
                     at_barrier->flat & 63u, at_barrier->file, at_barrier->line, first->flat & 63u);
            report(EXIT_COLLECTIVE_AND_BARRIER, text, first->file, first->line);
        }
        WaveSnap& snap = g_run.waves[w];
        snap.present = 0;
        for (unsigned i = lo; i < hi; i++) {
            LaneCtx& l = g_run.lanes[i];
            snap.vals[i - lo] = 0;
            if (l.state != AT_COLLECTIVE) continue;
            snap.vals[i - lo] = l.posted;
            snap.present |= 1ull << (i - lo);
            l.state = READY;
        }
    }
}

inline void run_group(unsigned n_lanes, dim3 block) {
    GroupRun& G = g_run;
    if (G.stacks_lanes < n_lanes) {
        if (G.stacks) munmap(G.stacks, G.stacks_lanes * kStackBytes);
        G.stacks = (char*)mmap(nullptr, (size_t)n_lanes * kStackBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (G.stacks == (char*)MAP_FAILED) report(EXIT_MODEL, "no memory for the lanes' stacks", __FILE__, __LINE__);
        G.stacks_lanes = n_lanes;
    }
    G.lanes.resize(n_lanes);
    G.waves.resize((n_lanes + 63) / 64);
    for (unsigned i = 0; i < n_lanes; i++) {
        LaneCtx& l = G.lanes[i];
        getcontext(&l.ctx);
        l.ctx.uc_stack.ss_sp = G.stacks + (size_t)i * kStackBytes;
        l.ctx.uc_stack.ss_size = kStackBytes;
        l.ctx.uc_link = nullptr;
        makecontext(&l.ctx, lane_entry, 0);
        l.state = READY;
        l.flat = i;
        l.tid = dim3(i % block.x, i / block.x % block.y, i / block.x / block.y);
        l.file = nullptr;
        l.line = 0;
    }
    const unsigned n_waves = (unsigned)G.waves.size();
    std::vector<unsigned> ord;
    for (;;) {
        make_order(ord, n_waves);
        for (unsigned w : ord) run_wave(w, n_lanes);
        const LaneCtx* first = nullptr;
        unsigned ready = 0;
        for (const LaneCtx& l : G.lanes) {
            if (l.state == READY) ready++;
            if (l.state != AT_BARRIER) continue;
            if (!first) first = &l;
            else if (first->line != l.line || strcmp(first->file, l.file)) {
                char text[200];
                snprintf(text, sizeof text, "threads %u and %u wait at barriers of different call sites, the other %s:%d,", first->flat, l.flat,
                         first->file, first->line);
                report(EXIT_BARRIER_SITES, text, l.file, l.line);
            }
        }
        if (!first) {
            if (ready) report(EXIT_STUCK, "a workgroup in which nothing can run and not everything has ended", "?", 0);
            return;
        }
        if (ready) report(EXIT_STUCK, "a workgroup in which nothing can run and not everything has ended", first->file, first->line);
        for (LaneCtx& l : G.lanes)
            if (l.state == AT_BARRIER) l.state = READY;
    }
}

// ---- LDS: the writable function-local statics of the launched kernel
struct Sym { std::string name; uintptr_t addr; size_t size; bool func, writable; };

inline const std::vector<Sym>& symbols() {
    static std::vector<Sym> all;
    static bool done = false;
    if (done) return all;
    done = true;
    uintptr_t base = 0;
    dl_iterate_phdr([](struct dl_phdr_info* info, size_t, void* p) { *(uintptr_t*)p = info->dlpi_addr; return 1; }, &base);
    FILE* f = fopen("/proc/self/exe", "rb");
    if (!f) return all;
    std::vector<char> img;
    char chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) img.insert(img.end(), chunk, chunk + got);
    fclose(f);
    if (img.size() < sizeof(ElfW(Ehdr))) return all;
    ElfW(Ehdr) eh;
    memcpy(&eh, img.data(), sizeof eh);
    if (memcmp(eh.e_ident, ELFMAG, SELFMAG) || eh.e_shentsize != sizeof(ElfW(Shdr)) ||
        eh.e_shoff + (size_t)eh.e_shnum * sizeof(ElfW(Shdr)) > img.size())
        return all;
    std::vector<ElfW(Shdr)> sh(eh.e_shnum);
    memcpy(sh.data(), img.data() + eh.e_shoff, sh.size() * sizeof(ElfW(Shdr)));
    for (const ElfW(Shdr)& s : sh) {
        if (s.sh_type != SHT_SYMTAB || s.sh_link >= sh.size()) continue;
        const ElfW(Shdr)& str = sh[s.sh_link];
        if (s.sh_offset + s.sh_size > img.size() || str.sh_offset + str.sh_size > img.size()) continue;
        for (size_t at = 0; at + sizeof(ElfW(Sym)) <= s.sh_size; at += sizeof(ElfW(Sym))) {
            ElfW(Sym) y;
            memcpy(&y, img.data() + s.sh_offset + at, sizeof y);
            const int type = ELF64_ST_TYPE(y.st_info);
            if ((type != STT_OBJECT && type != STT_FUNC) || y.st_shndx == SHN_UNDEF || y.st_shndx >= sh.size() || y.st_name >= str.sh_size) continue;
            const char* name = img.data() + str.sh_offset + y.st_name;
            all.push_back(Sym{std::string(name, strnlen(name, str.sh_size - y.st_name)), base + y.st_value, (size_t)y.st_size, type == STT_FUNC,
                              (sh[y.st_shndx].sh_flags & SHF_WRITE) != 0});
        }
    }
    return all;
}

struct LdsBlock { char* p; size_t n; };

// the function-local statics of the function at `fn`: a local `x` of _Z<encoding> is _ZZ<encoding>E1x (or ..._<n> further down)
inline std::vector<LdsBlock> lds_of(const void* fn) {
    std::vector<LdsBlock> out;
    const std::vector<Sym>& all = symbols();
    if (all.empty()) report(EXIT_MODEL, "the program has no symbol table: a kernel's LDS cannot be found", __FILE__, __LINE__);
    for (const Sym& k : all) {
        if (!k.func || k.addr != (uintptr_t)fn || k.name.compare(0, 2, "_Z")) continue;
        const std::string prefix = "_ZZ" + k.name.substr(2) + "E";
        for (const Sym& v : all)
            if (!v.func && v.writable && v.size && !v.name.compare(0, prefix.size(), prefix)) out.push_back(LdsBlock{(char*)v.addr, v.size});
        return out;
    }
    // (a kernel without LDS gives an empty list above; a kernel that cannot be found would keep its LDS from workgroup to workgroup)
    report(EXIT_MODEL, "the launched kernel has no C++ function symbol in the program's symbol table: its LDS cannot be found", __FILE__, __LINE__);
}

HIP_LANES_NO_ASAN inline void fill_lds(const std::vector<LdsBlock>& blocks, uint64_t s) {
    for (const LdsBlock& b : blocks)
        for (size_t i = 0; i < b.n; i++) {
            if (!(i & 7)) s = next_random(s) | 1;
            b.p[i] = (char)(s >> (8 * (i & 7)));
        }
}

template <typename Kernel, typename... Args>
void launch_waves(Kernel kernel, dim3 grid, dim3 block, const Args&... args) {
    const uint64_t groups = (uint64_t)grid.x * grid.y * grid.z;
    const unsigned n_lanes = block.x * block.y * block.z;
    gridDim = grid;
    blockDim = block;
    launches++;
    lanes_run += groups * n_lanes;
    if (!groups || !n_lanes) return;
    static_assert(std::is_pointer<Kernel>::value, "a kernel is launched by its function");
    const std::vector<LdsBlock> lds = lds_of((const void*)kernel);
    auto body = [&] { kernel(args...); };
    g_run.body = [](void* p) { (*(decltype(body)*)p)(); };
    g_run.body_arg = &body;
    g_run.rng = seed * 3 + launches;
    std::vector<uint32_t> perm(groups);         // (a launch of this project's tests stays far below 2^32 workgroups)
    for (uint64_t i = 0; i < groups; i++) perm[i] = (uint32_t)(order == DESCENDING ? groups - 1 - i : i);
    if (order == SHUFFLED) {
        uint64_t s = seed + launches;
        for (uint64_t i = groups; i > 1; i--) std::swap(perm[i - 1], perm[next_random(s) % i]);
    }
    for (uint64_t i = 0; i < groups; i++) {
        uint64_t at = perm[i];
        blockIdx.x = (unsigned)(at % grid.x); at /= grid.x;
        blockIdx.y = (unsigned)(at % grid.y); at /= grid.y;
        blockIdx.z = (unsigned)at;
        fill_lds(lds, (seed + 0x51ED * (uint64_t)order) * 0x9E3779B97F4A7C15ull + launches * 0x10001 + perm[i]);
        run_group(n_lanes, block);
    }
}

// ---- the operations
template <typename T> uint64_t to_bits(T v) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "shuffles move 32- and 64-bit values");
    uint64_t b = 0;
    memcpy(&b, &v, sizeof v);
    return b;
}
template <typename T> T of_bits(uint64_t b) {
    T v;
    memcpy(&v, &b, sizeof v);
    return v;
}

template <typename T> T shfl(T v, int src, int width, const char* file, int line) {
    const WaveSnap& w = collective(to_bits(v), file, line);
    const int me = (int)lane_id();
    const int from = width >= 64 ? (src & 63) : (me & ~(width - 1)) | (src & (width - 1));
    return of_bits<T>(from_lane(w, from, "__shfl", file, line));
}
template <typename T> T shfl_up(T v, unsigned d, int width, const char* file, int line) {
    const WaveSnap& w = collective(to_bits(v), file, line);
    const int me = (int)lane_id(), in = me & (width - 1);
    if ((unsigned)in < d) return v;
    return of_bits<T>(from_lane(w, me - (int)d, "__shfl_up", file, line));
}
template <typename T> T shfl_down(T v, unsigned d, int width, const char* file, int line) {
    const WaveSnap& w = collective(to_bits(v), file, line);
    const int me = (int)lane_id(), in = me & (width - 1);
    if ((unsigned)in + d >= (unsigned)width) return v;
    return of_bits<T>(from_lane(w, me + (int)d, "__shfl_down", file, line));
}
template <typename T> T shfl_xor(T v, int mask, int width, const char* file, int line) {
    const WaveSnap& w = collective(to_bits(v), file, line);
    const int me = (int)lane_id(), in = (me & (width - 1)) ^ mask;
    if (in < 0 || in >= width) return v;
    return of_bits<T>(from_lane(w, (me & ~(width - 1)) | in, "__shfl_xor", file, line));
}

inline uint64_t ballot(bool p, const char* file, int line) {
    const WaveSnap& w = collective(p ? 1u : 0u, file, line);
    uint64_t m = 0;
    for (int i = 0; i < 64; i++)
        if (((w.present >> i) & 1ull) && w.vals[i]) m |= 1ull << i;
    return m;
}

inline int readlane(int v, int src, const char* file, int line) {
    const WaveSnap& w = collective((uint32_t)v, file, line);
    return (int)(uint32_t)from_lane(w, src, "readlane", file, line);
}
inline int readfirstlane(int v, const char* file, int line) {
    const WaveSnap& w = collective((uint32_t)v, file, line);
    return (int)(uint32_t)w.vals[__builtin_ctzll(w.present)];      // (the calling lane is present: never zero)
}

// v_mov_b32 with a DPP control, as the "Data Parallel Primitives" section of the CDNA3 / CDNA4 instruction set guides defines it
// (rows are 16 lanes, banks 4 lanes of a row): the lane takes src of the lane the control names; a lane whose row or bank is masked
// out, or whose source lies outside its row (row_shl / row_shr) while bound_ctrl is off, keeps `old`; with bound_ctrl on such a
// source reads as zero.  A lane in a row that row_bcast does not reach (row 0 for row_bcast:15, rows 0 and 1 for row_bcast:31) reads
// its own src when its row is enabled: that is what the MI355X does (tests/test_gpu_wave_probe.py), and why wave_ops.h masks
// those rows out.
inline int update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl, const char* file = __builtin_FILE(),
                      int line = __builtin_LINE()) {
    const WaveSnap& w = collective((uint32_t)src, file, line);
    const int me = (int)lane_id(), row = me >> 4, in_row = me & 15;
    int from = -1;                                                   // -1: no source
    if (ctrl >= 0x000 && ctrl <= 0x0FF) from = (me & ~3) | ((ctrl >> (2 * (me & 3))) & 3);                  // quad_perm
    else if (ctrl >= 0x101 && ctrl <= 0x10F) from = in_row + (ctrl & 15) <= 15 ? me + (ctrl & 15) : -1;    // row_shl
    else if (ctrl >= 0x111 && ctrl <= 0x11F) from = in_row >= (ctrl & 15) ? me - (ctrl & 15) : -1;         // row_shr
    else if (ctrl >= 0x121 && ctrl <= 0x12F) from = (me & ~15) | ((in_row - (ctrl & 15)) & 15);            // row_ror
    else if (ctrl == 0x140) from = (me & ~15) | (15 - in_row);                                              // row_mirror
    else if (ctrl == 0x141) from = (me & ~7) | (7 - (me & 7));                                              // row_half_mirror
    else if (ctrl == 0x142) from = row > 0 ? row * 16 - 1 : me;                                             // row_bcast:15
    else if (ctrl == 0x143) from = row > 1 ? 31 : me;                                                       // row_bcast:31
    else report(EXIT_MODEL, "a DPP control the stand-in does not know", file, line);
    if (!((row_mask >> row) & 1) || !((bank_mask >> (in_row >> 2)) & 1)) return old;
    if (from < 0) return bound_ctrl ? 0 : old;
    return (int)(uint32_t)from_lane(w, from, "DPP read", file, line);
}

inline uint32_t mbcnt_lo(uint32_t mask, uint32_t base) {
    const unsigned me = lane_id();
    return base + (uint32_t)__builtin_popcount(me >= 32 ? mask : mask & ((1u << me) - 1u));
}
inline uint32_t mbcnt_hi(uint32_t mask, uint32_t base) {
    const unsigned me = lane_id();
    return base + (uint32_t)__builtin_popcount(me <= 32 ? 0u : mask & ((1u << (me - 32)) - 1u));
}

}  // namespace hip_lanes

// ---- HIP's names
#define __shared__ static
#define __constant__ static
#define HIP_SYMBOL(x) (&(x))

inline void __syncthreads(const char* file = __builtin_FILE(), int line = __builtin_LINE()) { hip_lanes::barrier(file, line); }

#define HIP_LANES_SHFL(name, impl, idx_t)                                                                                                  \
    template <typename T>                                                                                                                  \
    inline T name(T v, idx_t a, int width = 64, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {                        \
        return hip_lanes::impl(v, a, width, file, line);                                                                                   \
    }
HIP_LANES_SHFL(__shfl, shfl, int)
HIP_LANES_SHFL(__shfl_up, shfl_up, unsigned)
HIP_LANES_SHFL(__shfl_down, shfl_down, unsigned)
HIP_LANES_SHFL(__shfl_xor, shfl_xor, int)
#undef HIP_LANES_SHFL

inline unsigned long long __ballot(int p, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    return hip_lanes::ballot(p != 0, file, line);
}
inline int __any(int p, const char* file = __builtin_FILE(), int line = __builtin_LINE()) { return hip_lanes::ballot(p != 0, file, line) != 0; }
inline int __all(int p, const char* file = __builtin_FILE(), int line = __builtin_LINE()) { return hip_lanes::ballot(p == 0, file, line) == 0; }
inline uint64_t hip_lanes_ballot_w64(bool p, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    return hip_lanes::ballot(p, file, line);
}
inline int hip_lanes_readlane(int v, int src, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    return hip_lanes::readlane(v, src, file, line);
}
inline int hip_lanes_readfirstlane(int v, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    return hip_lanes::readfirstlane(v, file, line);
}
#define __builtin_amdgcn_ballot_w64 hip_lanes_ballot_w64
#define __builtin_amdgcn_readlane hip_lanes_readlane
#define __builtin_amdgcn_readfirstlane hip_lanes_readfirstlane
#define __builtin_amdgcn_update_dpp hip_lanes::update_dpp
#define __builtin_amdgcn_mbcnt_lo hip_lanes::mbcnt_lo
#define __builtin_amdgcn_mbcnt_hi hip_lanes::mbcnt_hi

inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int __popc(unsigned v) { return __builtin_popcount(v); }
inline int __ffsll(unsigned long long v) { return __builtin_ffsll((long long)v); }
inline int __ffsll(long long v) { return __builtin_ffsll(v); }
inline int __clzll(long long v) { return v ? __builtin_clzll((unsigned long long)v) : 64; }

// atomics: lanes never overlap here, so each is the plain operation; the old value is returned
template <typename T, typename U> inline T atomicAdd(T* p, U v) { const T o = *p; *p = (T)(o + (T)v); return o; }
template <typename T, typename U> inline T atomicSub(T* p, U v) { const T o = *p; *p = (T)(o - (T)v); return o; }
template <typename T, typename U> inline T atomicMin(T* p, U v) { const T o = *p; if ((T)v < o) *p = (T)v; return o; }
template <typename T, typename U> inline T atomicMax(T* p, U v) { const T o = *p; if ((T)v > o) *p = (T)v; return o; }
template <typename T, typename U> inline T atomicOr(T* p, U v) { const T o = *p; *p = (T)(o | (T)v); return o; }
template <typename T, typename U> inline T atomicAnd(T* p, U v) { const T o = *p; *p = (T)(o & (T)v); return o; }
template <typename T, typename U> inline T atomicExch(T* p, U v) { const T o = *p; *p = (T)v; return o; }

struct alignas(8) uint2 { uint32_t x, y; };
inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
template <typename T> inline T min(T a, T b) { return b < a ? b : a; }
template <typename T> inline T max(T a, T b) { return a < b ? b : a; }
