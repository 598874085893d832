// wave_cursor.hpp — how a persistent wave takes its work from a stream of n entries, written once for every kernel that does.
// A wave owns a STATIC first run of entries, picked by its index in the grid with no atomic (thousands of waves starting together would
// queue ~90 us on the head word), and reserves further CHUNKS behind the grid's static part with one atomic each through a head word.
//   DealCursor    deals the entries of its run to the wave's IDLE lanes by ballot prefix, as many per step as lanes are idle
//                 (the laboratory's k_trace_pool and k_trace_pair; its statements in k_trace_vote, k_trace_shadow, k_finish: below)
//   StrideCursor  hands out 64 entries per trip, one per lane (k_shade_media, k_media_tail; its statements in k_shade_stream)
// The wave-uniform arithmetic of both (namespace cursor) is plain integer code, compiled for the device and — by
// tests/tools/wave_cursor_driver.cpp — for the host (tests/test_wave_cursor_cpu.py); ballot, atomic and readfirstlane stay in the structs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "wave.hpp"
#define VPT_CURSOR_HD __host__ __device__ inline
#else
#define VPT_CURSOR_HD static inline
#endif

namespace vpt {

// One atomic on a single word costs ~11 ns under contention (MI355X_MICROARCH.md 'dequeue': a head word
// saturates at ~88 dequeues/us), so the number of fetches per launch is kept near 8k: a wave takes
// n/8192 queue entries per fetch, rounded up to whole waves, between 64 and 1024.
constexpr uint32_t kFetchChunkMax = 1024u;
VPT_CURSOR_HD uint32_t fetch_chunk(uint32_t n) {
    uint32_t c = ((n >> 13) + 63u) & ~63u;
    return c < 64u ? 64u : (c > kFetchChunkMax ? kFetchChunkMax : c);
}

namespace cursor {
// entries the grid's waves own without an atomic; the head word counts from behind them
VPT_CURSOR_HD uint32_t static_part(uint32_t waves, uint32_t per_wave) { return waves * per_wave; }
// a run of `len` entries from `first`, cut short by the end of the stream
VPT_CURSOR_HD uint32_t run_end(uint32_t first, uint32_t len, uint32_t n) { return first + len < n ? first + len : n; }
// where the chunk begins that the head word's old value `reserved` stands for (at or beyond n: the stream is exhausted)
VPT_CURSOR_HD uint32_t chunk_first(uint32_t n_static, uint32_t reserved) { return n_static + reserved; }
// DealCursor: `want` idle lanes were offered entries from [next, end)
VPT_CURSOR_HD uint32_t deal_advance(uint32_t next, uint32_t end, uint32_t want) {
    const uint32_t left = end - next;
    return next + (want < left ? want : left);
}
// StrideCursor: no entry lies behind the static part of `active` waves
VPT_CURSOR_HD bool stride_static_only(uint32_t active, uint32_t n) { return active * 64u >= n; }
}  // namespace cursor

#if defined(__HIPCC__)
// Every member is called by every lane of the wave; every field is wave-uniform and lives in scalar registers.
//
// The product's k_trace_vote, k_trace_shadow and k_finish carry DealCursor's statements written out on LOCAL SCALARS (w_next, w_end, exhausted),
// as they were before this header, and k_shade_stream StrideCursor's, instead of holding the struct.  The compiler promotes a kernel's locals to registers
// BEFORE it inlines anything (sroa ahead of the inliner in the -O3 pipeline); a local whose address goes into a call — `this` of a member, a
// reference parameter, a lambda's capture — waits for the round after inlining, comes out at another place among the loop's values, and the
// register allocation of the whole kernel follows: those kernels then no longer compile to the machine code that was measured
// (profiles/wave_cursor_asm_identity.md; even cursor::run_end, by value, inside the refill branch does that).  A kernel that
// is new, or whose allocation is open anyway, takes the structs.
struct DealCursor {
    bool exhausted;
    uint32_t end, next, n_static, chunk, n;
    // waves_per_block: of the kernel's launch bound, a constant (blockDim would be a load)
    __device__ __forceinline__ DealCursor(uint32_t n_, uint32_t per_wave, uint32_t chunk_, uint32_t waves_per_block) {
        n = n_; chunk = chunk_;
        n_static = cursor::static_part(gridDim.x * waves_per_block, per_wave);
        next = __builtin_amdgcn_readfirstlane((blockIdx.x * waves_per_block + (threadIdx.x >> 6)) * per_wave);
        end = cursor::run_end(next, per_wave, n);
        if (next >= n) { next = 0u; end = 0u; }
        exhausted = false;
    }
    // make sure there is a run to deal from: the next chunk through `head` when this one is used up; sets `exhausted` when the stream is
    __device__ __forceinline__ void refill(uint32_t* head) {
        if (next >= end) {
            if (n_static >= n) exhausted = true;
            else {
                uint32_t base = 0u;
                if (lane_id() == 0u) base = atomicAdd(head, chunk);
                base = cursor::chunk_first(n_static, __builtin_amdgcn_readfirstlane(base));
                if (base >= n) exhausted = true;
                else { next = base; end = cursor::run_end(base, chunk, n); }
            }
        }
    }
    // the entry of this lane, given the ballot of idle lanes: the lane takes it if it is idle and the index < end ...
    __device__ __forceinline__ uint32_t index(unsigned long long m_idle) const { return next + lanes_below(m_idle); }
    // ... and the run moves on by what was taken
    __device__ __forceinline__ void advance(unsigned long long m_idle) { next = cursor::deal_advance(next, end, (uint32_t)__popcll(m_idle)); }
};

struct StrideCursor {
    uint32_t pos, end, n, active, chunk;
    bool done;
    // gw: the wave's index in the grid, wave-uniform (readfirstlane) for the reason above; active: waves that take part, min(grid, ceil(n / 64))
    __device__ __forceinline__ void init(uint32_t gw, uint32_t n_, uint32_t active_) {
        n = n_; active = active_; chunk = fetch_chunk(n_); pos = gw * 64u; end = pos + 64u; done = false;
    }
    // returns false when the stream is exhausted; otherwise `i` is this lane's entry (may be >= n: no entry)
    __device__ __forceinline__ bool next(uint32_t* head, uint32_t& i) {
        while (pos >= end || pos >= n) {
            if (done || cursor::stride_static_only(active, n)) { done = true; return false; }
            uint32_t nb = 0u;
            if (lane_id() == 0u) nb = atomicAdd(head, chunk);
            pos = cursor::chunk_first(active * 64u, __builtin_amdgcn_readfirstlane(nb));
            end = pos + chunk;
            if (pos >= n) { done = true; return false; }
        }
        i = pos + lane_id();
        pos += 64u;
        return true;
    }
};
#endif  // __HIPCC__

}  // namespace vpt
