// plane_ring.h -- the k loop of every split-plane GEMM of the library, stated once: planes_gemm_kernel and layer 0 of planes_chain4_kernel
// (planes.hip), dec_main_kernel_b3 (decoder.hip) and dec_main_h2_kernel (decoder_h2.hip).
//
//   A operand: weight planes, shared by the workgroup's four waves, through an LDS-DMA ring (WStreamT, mfma_chain.h);
//   B operand: the planes of the wave's NT row tiles, loaded by inline-assembly global_load_dwordx4 into SETS rotating register sets,
//              SETS - 1 k-steps ahead;
//   waits:     counted (s_waitcnt vmcnt(N)) at the ring boundaries, each NAMING the register set it covers.
// The callers own what surrounds the loop: the ring's first NB - 1 DMAs, the accumulators' initial value (bias) and every epilogue.
#pragma once
#include "mfma_chain.h"

// The arithmetic of a planes kernel: P = 3 -> bf16x3 (three bf16 planes per operand, six products), P = 2 -> f16x2 (two fp16 planes of the
// operand times an exact power of two, three products; mfma_chain.h).  pa(q) / pb(q): the A and B plane of product q, smallest first.
template <int P> struct PgArith;
template <> struct PgArith<3> {
    typedef bf16x8 vec;
    static constexpr int NQ = 6;
    static __device__ __forceinline__ constexpr int pa(int q) { return q == 0 ? 2 : (q == 1 ? 0 : (q == 2 ? 1 : (q == 3 ? 1 : 0))); }   // (lo,hi) (hi,lo) (mid,mid)
    static __device__ __forceinline__ constexpr int pb(int q) { return q == 0 ? 0 : (q == 1 ? 2 : (q == 2 ? 1 : (q == 3 ? 0 : (q == 4 ? 1 : 0)))); }   // (mid,hi) (hi,mid) (hi,hi)
    static __device__ __forceinline__ void split(const f32x4 &a, const f32x4 &b, float, vec (&pl)[3]) { b3_split8(a, b, pl); }
    static __device__ __forceinline__ f32x4 mfma(const vec &a, const vec &b, const f32x4 &c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct PgArith<2> {
    typedef f16x8 vec;
    static constexpr int NQ = 3;
    static __device__ __forceinline__ constexpr int pa(int q) { return q == 0 ? 1 : 0; }      // smallest first: (lo,hi) (hi,lo) (hi,hi)
    static __device__ __forceinline__ constexpr int pb(int q) { return q == 1 ? 1 : 0; }
    static __device__ __forceinline__ void split(const f32x4 &a, const f32x4 &b, float rho, vec (&pl)[2]) { h2_split8(a, b, rho, pl); }
    static __device__ __forceinline__ f32x4 mfma(const vec &a, const vec &b, const f32x4 &c) { return H2_MFMA(a, b, c); }
};

__device__ __forceinline__ uint4 pg_load_async(const uint4 *p)    // placed exactly here; completion rides on the ring's s_waitcnt
{
    uint4 v;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    return v;
}

// A counted wait that covers the register set about to be CONSUMED: the set goes through the statement as read-write operands, so no
// instruction that uses the loaded values can be scheduled above the wait (a "memory" clobber does not order register arithmetic: the
// compiler hoisted a conversion of gathered rows above a bare s_waitcnt once the register allocation shifted), and the registers stay
// allocated to the set until it.  Sets still in flight are untouched until their own wait (or the final drain) names them.
// (Operands as native vectors: a HIP_vector_type is an aggregate the constraint cannot take.  NT x NBV = 4, 6, 8 or 12 of them.)
typedef unsigned int pg_u32x4 __attribute__((ext_vector_type(4)));
#define PG_RW2(r, o) "+v"(r[o]), "+v"(r[o + 1])
#define PG_RW4(r, o) PG_RW2(r, o), PG_RW2(r, o + 2)
template <int N, int NT, int NBV>
__device__ __forceinline__ void pg_wait_set(uint4 (&b)[NT][NBV])
{
    constexpr int NR = NT * NBV;
    static_assert(NR == 4 || NR == 6 || NR == 8 || NR == 12, "2 or 4 tiles of 2 or 3 planes");
    pg_u32x4 r[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) r[i] = __builtin_bit_cast(pg_u32x4, b[i / NBV][i % NBV]);
    if constexpr (NR == 4) asm volatile("s_waitcnt vmcnt(%4)" : PG_RW4(r, 0) : "n"(N) : "memory");
    else if constexpr (NR == 6) asm volatile("s_waitcnt vmcnt(%6)" : PG_RW4(r, 0), PG_RW2(r, 4) : "n"(N) : "memory");
    else if constexpr (NR == 8) asm volatile("s_waitcnt vmcnt(%8)" : PG_RW4(r, 0), PG_RW4(r, 4) : "n"(N) : "memory");
    else asm volatile("s_waitcnt vmcnt(%12)" : PG_RW4(r, 0), PG_RW4(r, 4), PG_RW4(r, 8) : "n"(N) : "memory");
#pragma unroll
    for (int i = 0; i < NR; ++i) b[i / NBV][i % NBV] = __builtin_bit_cast(uint4, r[i]);
}
#undef PG_RW4
#undef PG_RW2

// The end of a k loop: wait for every load still in flight -- the B loads of the last SETS - 1 (clamped, unused) k-steps among them --
// with EVERY rotating register set named by the wait.  The compiler does not know that an asm load's result arrives later: on paths
// where a set's value is dead (a layer with one or two k-steps never reads the third set; after the last k-step all sets are dead) it
// would hand the registers to something else while the load is still in flight, and the data landing afterwards would overwrite that
// something (found by tools/asm_load_lint.py on the f16x2 chain of sa1, one k-step: the next layer's operand planes were built in
// those registers -- results changed from call to call).  Tied to a wait, the sets stay allocated until their loads have landed.
// One statement per set (three sets of four tiles x three planes are 36 operands, more than one statement takes); the first one waits.
template <int SETS, int NT, int NBV>
__device__ __forceinline__ void pg_drain_loads(uint4 (&bs)[SETS][NT][NBV])
{
#pragma unroll
    for (int s = 0; s < SETS; ++s) pg_wait_set<0, NT, NBV>(bs[s]);
}

// The barrier of a ring boundary WITHOUT __syncthreads()' fences.  The release fence in __syncthreads() makes the compiler wait for
// EVERY outstanding vector-memory operation (s_waitcnt vmcnt(0)) in front of the s_barrier -- LDS-DMA fills are tracked by vmcnt and
// write LDS, so it cannot tell them from the plane loads -- which throws away the counted waits above it: the plane loads of k-step
// t + 2 and the ring fills of the next chunks, issued to stay in flight across the boundary, were all drained at every boundary
// (matrix pipe 0.43 busy in the 512 -> 1024 layer; the f16x2 decoder: 6.01 / 6.07 -> 5.92 / 5.99 ms per 1024 clouds,
// tools/experiments/r5/README.md).  What the protocol needs is already explicit: each wave's counted wait covers its own
// pieces of chunk c (in-order completion), the barrier then says everyone's have landed and everyone has finished reading chunk c - 1
// (those reads feed MFMAs issued before the barrier; the compiler's own lgkmcnt wait for them precedes their use).
// BARE = false keeps __syncthreads(): the bf16x3 planes forms, the one-chunk forms and the chains gain nothing measurable from the bare
// barrier, and with the compiler's drain in place tools/asm_load_lint.py can check them.
template <bool BARE>
__device__ __forceinline__ void pg_ring_barrier()
{
    if constexpr (BARE) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    } else {
        __syncthreads();
    }
}

// DMA of chunk c of the stream.  A chunk past the end re-reads chunk 0 into a free buffer, so every boundary issues the same loads and
// the counted waits hold to the last k-step.
template <class WS>
__device__ __forceinline__ void pg_ring_issue(const WS &ws, int c) { ws.issue(c < ws.nch ? c : 0, c % WS::buffers); }

// VMEM issue order per wave.  A k-step is HALVES ring chunks; boundary b (= HALVES t + half) issues the DMA of chunk b + NB - 1 [DMA
// loads] and, when half == 0, the B planes of k-step t + SETS - 1 [NBL loads] after it.  Loads complete in order, so a boundary may
// leave in flight everything issued after the youngest load it needs:
//   chunk b's DMA, the first thing issued at boundary b - (NB - 1), and
//   half == 0: the B planes of k-step t, the last thing issued at boundary b - HALVES (SETS - 1).
// pg_keep counts those younger loads.  The four users: HALVES = 2, NB = 4, three sets: 2 DMA + NBL and 2 DMA + 2 NBL;
// two sets: DMA and 2 DMA + 2 NBL;  HALVES = 1 (NB = 3 or 4), three sets: DMA + NBL.
constexpr int pg_keep(int HALVES, int NB, int SETS, int DMA, int NBL, int half)
{
    int after_dma = 0;
    for (int j = 1; j < NB; ++j) after_dma += (j < NB - 1 ? DMA : 0) + ((j - half) % HALVES == 0 ? NBL : 0);      // boundary b - j
    if (half != 0) return after_dma;
    int after_b = 0;
    for (int j = 1; j < HALVES * (SETS - 1); ++j) after_b += DMA + (j % HALVES == 0 ? NBL : 0);
    return after_b < after_dma ? after_b : after_dma;
}
static_assert(pg_keep(2, 4, 3, 3, 6, 0) == 2 * 3 + 6 && pg_keep(2, 4, 3, 3, 6, 1) == 2 * 3 + 2 * 6, "bf16x3, two chunks per k-step: 12 and 18");
static_assert(pg_keep(2, 4, 2, 2, 8, 0) == 2 && pg_keep(2, 4, 2, 2, 8, 1) == 2 * 2 + 2 * 8, "f16x2 decoder, four tiles in two sets: 2 and 20");
static_assert(pg_keep(1, 4, 3, 3, 6, 0) == 3 + 6 && pg_keep(1, 3, 3, 4, 4, 0) == 4 + 4, "one chunk per k-step: DMA + NBL");

// acc[nt][m] += sum over the KT k-steps (KT_FIXED when > 0, else the runtime kt) of the products of PgArith<P>, for the NT row tiles of the
// wave and the HALVES x MQC m-tiles of the workgroup's m-block.
//   ws     the weight ring, chunk = MQC m-tiles x P planes; chunk c of the stream belongs to k-step c / HALVES.  The caller has issued
//          the DMAs of chunks 0 .. NB - 2 (pg_ring_issue).
//   baddr  (nt, pl, t) -> address of this lane's 16 bytes of B plane pl of tile nt at k-step t (t < KT: later k-steps repeat the last).
//   SPLIT  the two "planes" are raw fp32 (channels 4 g .. + 3 of both halves of the k-step, gathered rows) and are split into the P
//          operand planes, times rho, when the k-step consumes them (4 loads per k-step and tile pair instead of 2 P).
// A fragments are read from LDS four m-tiles at a time; the products of a group run smallest first over 4 m-tiles x NT tiles.
template <int P, int NT, int SETS, int MQC, int HALVES, bool BARE, int KT_FIXED, bool SPLIT, class WS, class BAddr>
__device__ __forceinline__ void pg_ring_gemm(const WS &ws, int kt, const BAddr &baddr, float rho, f32x4 (&acc)[NT][HALVES * MQC])
{
    typedef PgArith<P> AR;
    typedef typename AR::vec avec;
    constexpr int NB = WS::buffers, DMA = WS::chunk_frags / 4;            // ring depth; LDS-DMA loads per wave and chunk
    constexpr int NBV = SPLIT ? 2 : P, NBL = NT * NBV;                    // B registers per tile; B loads per k-step
    constexpr bool FIXED = KT_FIXED > 0;
    static_assert(WS::chunk_frags == MQC * P && MQC % 4 == 0 && NB >= 3 && (SETS == 2 || SETS == 3), "ring geometry");
    static_assert(!FIXED || (KT_FIXED >= 2 && (KT_FIXED - 2) % SETS == 0), "a fixed K runs whole trips of the rotation");
    const int KT = FIXED ? KT_FIXED : kt;
    uint4 bs[SETS][NT][NBV];
    auto load_b = [&](uint4 (&dst)[NT][NBV], int t) {
        const int tc = t < KT ? t : KT - 1;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int pl = 0; pl < NBV; ++pl) dst[nt][pl] = pg_load_async(baddr(nt, pl, tc));
    };
    auto kstep = [&](int t, uint4 (&braw)[NT][NBV], uint4 (&bload)[NT][NBV], bool first) {
        avec bc[NT][P];
#pragma unroll
        for (int half = 0; half < HALVES; ++half) {
            const int c = HALVES * t + half;
            if (half == 0) {
                if (first) pg_wait_set<0, NT, NBV>(braw);                 // everything issued so far
                else pg_wait_set<pg_keep(HALVES, NB, SETS, DMA, NBL, 0), NT, NBV>(braw);
                pg_ring_barrier<BARE>();
                pg_ring_issue(ws, c + NB - 1);
                load_b(bload, t + SETS - 1);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    if constexpr (SPLIT)
                        AR::split(__builtin_bit_cast(f32x4, braw[nt][0]), __builtin_bit_cast(f32x4, braw[nt][1]), rho, bc[nt]);
                    else
#pragma unroll
                        for (int pl = 0; pl < P; ++pl) bc[nt][pl] = __builtin_bit_cast(avec, braw[nt][pl]);
                }
            } else {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(pg_keep(HALVES, NB, SETS, DMA, NBL, 1)) : "memory");       // covers a DMA only
                pg_ring_barrier<BARE>();
                pg_ring_issue(ws, c + NB - 1);
            }
            const f32x4 *buf = ws.chunk(c);
#pragma unroll
            for (int sub = 0; sub < MQC / 4; ++sub) {
                avec a[4][P];
#pragma unroll
                for (int mq = 0; mq < 4; ++mq)
#pragma unroll
                    for (int pl = 0; pl < P; ++pl) a[mq][pl] = __builtin_bit_cast(avec, buf[((4 * sub + mq) * P + pl) * 64]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < AR::NQ; ++q)
#pragma unroll
                    for (int mq = 0; mq < 4; ++mq)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[nt][MQC * half + 4 * sub + mq] = AR::mfma(a[mq][AR::pa(q)], bc[nt][AR::pb(q)], acc[nt][MQC * half + 4 * sub + mq]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // k-step t consumes set t % SETS and loads k-step t + SETS - 1 into set (t - 1) % SETS: SETS k-steps per trip, static register sets
#pragma unroll
    for (int s = 0; s < SETS - 1; ++s) load_b(bs[s], s);
    kstep(0, bs[0], bs[SETS - 1], true);
    if (FIXED || KT > 1) kstep(1, bs[1], bs[0], false);
#pragma unroll 1
    for (int t = 2; t < KT; t += SETS) {
#pragma unroll
        for (int j = 0; j < SETS; ++j)
            if (FIXED || j == 0 || t + j < KT) kstep(t + j, bs[(2 + j) % SETS], bs[(1 + j) % SETS], false);
    }
    pg_drain_loads<SETS, NT, NBV>(bs);                                    // the last (clamped, unused) B loads and the ring's DMAs
}
