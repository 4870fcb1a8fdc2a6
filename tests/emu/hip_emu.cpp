// tests/emu/hip_emu.cpp -- runtime of the CPU SIMT emulation (TEST INFRASTRUCTURE ONLY, see hip/hip_runtime.h)
//
// The lanes of a block are fibers on the launching thread, switched in user space: a wave operation (ballot, shuffle) or __syncthreads() is a
// barrier among 64 / all fibers, and a fiber that waits hands the processor to the next one.  (One operating-system thread per lane with
// pthread barriers, the first form of this file, spent nearly all of its time in futex calls: a ballot cost a hundred microseconds.)
// Blocks run one after the other, in order (static __shared__ storage; look-backs find their predecessors finished).  A wave operation
// inside divergent control flow, which hangs the GPU, is reported here: the scheduler sees that no fiber can move.
// HIPEMU_WAVES_APART (launch below) runs the waves of a block one at a time between barriers and poisons LDS at every block start.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <atomic>
#include <mutex>

#if defined(__SANITIZE_ADDRESS__)
extern "C" void __sanitizer_start_switch_fiber(void **fake_stack_save, const void *bottom, size_t size);
extern "C" void __sanitizer_finish_switch_fiber(void *fake_stack_save, const void **bottom_old, size_t *size_old);
#define EMU_ASAN 1
#else
#define EMU_ASAN 0
#endif

// void emu_switch(void **save_sp, void *load_sp): callee-saved registers of the System V x86-64 ABI on the old stack, then the new stack's
extern "C" void emu_switch(void **save_sp, void *load_sp);
asm(R"(
    .text
    .globl emu_switch
    .type emu_switch, @function
emu_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
    .size emu_switch, .-emu_switch
)");

namespace hipemu {
thread_local Idx t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;

namespace {
constexpr size_t STACK = (size_t)512 << 10, GUARD = 4096;
struct Fiber { void *sp; bool done, at_block; unsigned bar_gen; };      // at_block: arrived at the __syncthreads() of generation bar_gen
struct Barrier { unsigned arrived = 0, gen = 0; };
struct Run {
    Fiber fib[1024]; unsigned nt = 0, cur = 0; void *sched_sp = nullptr;
    Barrier block_bar, wave_bar[16];
    uint64_t wave_buf[16][64];
    std::vector<unsigned char> dyn;
    const std::function<void()> *fn = nullptr;
    bool progress = false;
    unsigned char *stacks = nullptr;      // 1024 stacks, mapped once
    const void *sched_bottom = nullptr; size_t sched_size = 0;      // (address sanitizer builds: the scheduler's stack, learnt at the first switch)
};
Run g;      // (one launch at a time: the mutex in launch())

unsigned char *stack_of(unsigned t) { return g.stacks + (size_t)t * (STACK + GUARD) + GUARD; }

void to_scheduler()
{
    Fiber &f = g.fib[g.cur];
#if EMU_ASAN
    void *fake = nullptr;
    __sanitizer_start_switch_fiber(f.done ? nullptr : &fake, g.sched_bottom, g.sched_size);
#endif
    emu_switch(&f.sp, g.sched_sp);
#if EMU_ASAN
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
}

void fiber_main()
{
#if EMU_ASAN
    __sanitizer_finish_switch_fiber(nullptr, &g.sched_bottom, &g.sched_size);
#endif
    (*g.fn)();
    g.fib[g.cur].done = true; g.progress = true;
    to_scheduler();
    abort();
}

void wait_at(Barrier &b, unsigned count)
{
    const unsigned gen = b.gen;
    if (++b.arrived == count) { b.arrived = 0; ++b.gen; g.progress = true; return; }
    while (b.gen == gen) to_scheduler();
}
bool waits_at_block(unsigned t) { return g.fib[t].at_block && g.fib[t].bar_gen == g.block_bar.gen; }

void run_fiber(unsigned t)
{
    g.cur = t; t_threadIdx = Idx{t, 0, 0};
#if EMU_ASAN
    void *fake = nullptr;
    __sanitizer_start_switch_fiber(&fake, stack_of(t), STACK);
#endif
    emu_switch(&g.sched_sp, g.fib[t].sp);
#if EMU_ASAN
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
}
} // namespace

// the static __shared__ storage of the kernels: tests/emu/lds.ld collects it between these two symbols (build.sh checks that it holds all of it;
// a library linked without the script has neither, and refuses HIPEMU_WAVES_APART)
extern "C" __attribute__((weak)) unsigned char hipemu_lds_begin[], hipemu_lds_end[];

void sync_block()
{
    Fiber &f = g.fib[g.cur];
    f.at_block = true; f.bar_gen = g.block_bar.gen;
    wait_at(g.block_bar, g.nt);
    f.at_block = false;
}
void sync_wave() { wait_at(g.wave_bar[t_threadIdx.x >> 6], 64); }
void yield() { to_scheduler(); }
uint64_t *wave_buf() { return g.wave_buf[t_threadIdx.x >> 6]; }
void *dyn_shared() { return g.dyn.data(); }

void launch(dim3 grid, dim3 block, size_t shmem, const std::function<void()> &fn, const char *kernel_name)
{
    const unsigned nt = block.x;
    if (nt == 0 || grid.x == 0) return;
    if (nt % 64 != 0 || nt > 1024) { fprintf(stderr, "hipemu: block size %u unsupported\n", nt); abort(); }
    static std::mutex one_launch;                 // static __shared__ storage, global barriers: one kernel at a time, whichever host thread launches
    std::lock_guard<std::mutex> lock(one_launch);
    if (!g.stacks) {
        g.stacks = (unsigned char *)mmap(nullptr, 1024 * (STACK + GUARD), PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (g.stacks == MAP_FAILED) { perror("hipemu: mmap"); abort(); }
        for (unsigned t = 0; t < 1024; ++t) mprotect(g.stacks + (size_t)t * (STACK + GUARD), GUARD, PROT_NONE);
    }
    g.dyn.assign(shmem + 64, 0);
    constexpr unsigned char LDS_POISON = 0xA5;
    g.nt = nt; g.fn = &fn;
    // HIPEMU_REVERSE=<kernel name>[,<kernel name>...]: the blocks of those kernels run from the last to the first, and so do the lanes of a
    // block.  Threads that are meant to be independent (one cluster of the left-justification each) must not care; run in index order only,
    // an overlap between two of them looks like the sequential algorithm and stays hidden (it did: dw_walk.hip reach_del, found on the GPU).
    // Not for kernels whose blocks wait for their predecessors (look-backs).
    // HIPEMU_REVERSE_LANES=<kernel names>: only the lanes (blocks stay in order): for kernels with look-backs; shows code that counts on the
    // lock step of a wave where no wave operation enforces it.
    auto named_in = [&](const char *var) {
        const char *e = getenv(var);
        if (!e) return false;
        const char *nm = kernel_name ? kernel_name : "";
        const char *colon = strrchr(nm, ':'); if (colon) nm = colon + 1;                  // dw::k_jrun -> k_jrun
        const size_t n = strcspn(nm, "<( ");
        for (const char *q = e; *q;) { const size_t m = strcspn(q, ","); if ((m == n && !strncmp(q, nm, n)) || (m == 3 && !strncmp(q, "all", 3))) return true; q += m; if (*q == ',') ++q; }
        return false;
    };
    const bool reverse_blocks = named_in("HIPEMU_REVERSE");
    const bool reverse_lanes = reverse_blocks || named_in("HIPEMU_REVERSE_LANES");
    // HIPEMU_WAVES_APART=<kernel names>|all: the waves of a block run one at a time -- a wave alone, its lanes round-robin, until every one of them has
    // finished or waits at __syncthreads(), then the next wave: the last wave first, or in an order shuffled per block by HIPEMU_WAVES_SEED=<n>.  Waves
    // are unordered between barriers on the GPU, so this is a legal schedule; under it the wave that runs first sees none of the other waves' stores
    // since the last barrier, and a missing barrier between a table's fill and its use shows every time.  LDS (static __shared__ and dynamic) is filled with the byte
    // LDS_POISON at every block start, as undefined as on the GPU.
    const bool apart = named_in("HIPEMU_WAVES_APART");
    const char *seed_env = getenv("HIPEMU_WAVES_SEED");
    if (apart && !hipemu_lds_begin) { fprintf(stderr, "hipemu: HIPEMU_WAVES_APART needs a library linked with tests/emu/lds.ld\n"); abort(); }
    const unsigned gy = grid.y ? grid.y : 1;
    const Idx saved[4] = {t_threadIdx, t_blockIdx, t_blockDim, t_gridDim};
    t_blockDim = Idx{nt, 1, 1}; t_gridDim = Idx{grid.x, gy, 1};
    for (unsigned y = 0; y < gy; ++y)
        for (unsigned bb = 0; bb < grid.x; ++bb) {      // blocks run one after the other (static __shared__ storage)
            const unsigned b = reverse_blocks ? grid.x - 1 - bb : bb;
            t_blockIdx = Idx{b, y, 0};
            g.block_bar = Barrier();
            for (unsigned w = 0; w < nt / 64; ++w) g.wave_bar[w] = Barrier();
            for (unsigned t = 0; t < nt; ++t) {
                void **top = (void **)(stack_of(t) + STACK);
                top[-2] = (void *)&fiber_main;            // return address of the first switch; the stack pointer is 8 mod 16 behind it, as after a call
                for (int k = 3; k <= 8; ++k) top[-k] = nullptr;
                g.fib[t].sp = (void *)(top - 8); g.fib[t].done = false; g.fib[t].at_block = false;
            }
            if (apart) {      // LDS is undefined at the start of a block
                memset(hipemu_lds_begin, LDS_POISON, (size_t)(hipemu_lds_end - hipemu_lds_begin));
                memset(g.dyn.data(), LDS_POISON, g.dyn.size());
            }
            const unsigned nw = nt / 64;
            unsigned wave_order[16];
            for (unsigned k = 0; k < nw; ++k) wave_order[k] = nw - 1 - k;            // the last wave first
            if (apart && seed_env) {
                uint64_t x = strtoull(seed_env, nullptr, 0) * 0x9E3779B97F4A7C15ull + ((uint64_t)y << 32 | b);
                for (unsigned k = nw; k > 1; --k) {                                   // Fisher-Yates with splitmix64
                    x += 0x9E3779B97F4A7C15ull;
                    uint64_t z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
                    const unsigned r = (unsigned)(z % k); const unsigned tmp = wave_order[k - 1]; wave_order[k - 1] = wave_order[r]; wave_order[r] = tmp;
                }
            }
            unsigned left = nt, idle_rounds = 0;
            while (left) {
                bool moved = false;
                if (apart) {
                    // one wave at a time, until each of its lanes has finished or waits at __syncthreads(); a wave whose lanes only poll (yield without
                    // a barrier completed or a lane finished) passes its turn
                    for (unsigned k = 0; k < nw; ++k) {
                        const unsigned w = wave_order[k];
                        for (;;) {
                            g.progress = false;
                            bool ran = false;
                            for (unsigned l = 0; l < 64; ++l) {
                                const unsigned t = w * 64 + (reverse_lanes ? 63 - l : l);
                                if (g.fib[t].done || waits_at_block(t)) continue;
                                ran = true;
                                run_fiber(t);
                                if (g.fib[t].done) --left;
                            }
                            if (!ran || !g.progress) break;
                            moved = true;
                        }
                    }
                } else {
                    g.progress = false;
                    for (unsigned tt = 0; tt < nt; ++tt) {
                        const unsigned t = reverse_lanes ? nt - 1 - tt : tt;
                        if (g.fib[t].done) continue;
                        run_fiber(t);
                        if (g.fib[t].done) --left;
                    }
                    moved = g.progress;
                }
                // no barrier completed, no lane finished: either lanes poll memory for one another (s_sleep loops), or some lanes wait at a wave
                // operation the others will never reach
                idle_rounds = moved ? 0 : idle_rounds + 1;
                if (idle_rounds > 100000) { fprintf(stderr, "hipemu: block %u: no lane can move -- a wave operation (ballot, shuffle, barrier) inside divergent control flow?\n", b); abort(); }
            }
        }
    t_threadIdx = saved[0]; t_blockIdx = saved[1]; t_blockDim = saved[2]; t_gridDim = saved[3];
}
} // namespace hipemu

// device and page-locked memory (hipMalloc / hipHostMalloc): live allocations are counted, and the k-th allocation from a given moment can be
// made to fail with hipErrorOutOfMemory -- tests/test_emu_memory.py checks that every allocation is freed and that a failed one leaves sound state
namespace {
std::atomic<long> g_live{0}, g_fail_in{0}, g_live_handles{0};
}
namespace hipemu {
hipError_t mem_alloc(void **p, size_t n)
{
    *p = nullptr;
    if (g_fail_in.load() > 0 && g_fail_in.fetch_sub(1) == 1) return hipErrorOutOfMemory;
    if (posix_memalign(p, 256, n ? n : 1) != 0) { *p = nullptr; return hipErrorOutOfMemory; }
    ++g_live;
    return hipSuccess;
}
void mem_free(void *p)
{
    if (!p) return;
    --g_live;
    free(p);
}
// streams and events (zeroed; never made to fail: the k-th ALLOCATION is what the tests fail)
void *handle_make(size_t n) { ++g_live_handles; return calloc(1, n); }
void handle_free(void *h)
{
    if (!h) return;
    --g_live_handles;
    free(h);
}
} // namespace hipemu
extern "C" long hipemu_live_allocs(void) { return g_live.load(); }
extern "C" long hipemu_live_handles(void) { return g_live_handles.load(); }      // streams + events created and not destroyed
// k > 0: the k-th allocation from now fails (once); 0: none.  Returns how many allocations the previous request still had to wait for (0: it fired or there was none).
extern "C" long hipemu_fail_alloc(long k) { return g_fail_in.exchange(k < 0 ? 0 : k); }
