// Attention for fp8 (OCP e4m3fn) KV caches: attnDecodeFp8Kernel for every decode row of a --kv-dtype
// fp8 engine, from a context of one key upward (there is no VALU kernel and no fused attention block
// for this type), and attnPrefillFp8Kernel (below it) for the row blocks of a prompt.
//
// Semantics: the cache holds e4m3fn(clamp(x, -448, 448)) of the rotated K and of V (qkvPairStore,
// decode_common.h); attention over an fp8 cache is attention over those stored values. The kernel
// widens each byte to bf16 in registers (exact: every e4m3 value is a bf16 value) and from there on
// is the arithmetic of attnDecodeMfmaKernel (attn_mfma.hip): Q . scale and P rounded to bf16,
// v_mfma_f32_16x16x32_bf16, f32 online softmax. So the fp8 cache costs the one rounding at append.
//
// Work split (attn_mfma.hip's): one workgroup per (row, KV head, key chunk), grid (nKvHeads, splitGrid,
// B), 256 threads; its 4 waves take the chunk's 64-key tiles round-robin (wave w: tiles w, w + 4, ...)
// in barrier-ordered rounds, each wave double-buffering its own K and V tiles in LDS. A key row is HS
// bytes, so a 64-key tile is 8 KB at head size 128 - the bf16 kernel's tile bytes, hence its bytes in
// flight per wave, its 8 + 8 LDS-DMA wave-instructions per tile and its vmcnt(16) - and 4 KB (4 + 4
// instructions, vmcnt(8)) at head size 64. One 16-byte-per-lane wave-instruction covers 8 (16) rows.
// Per tile a wave
//   * S^T = K . Q^T: MFMA rows = 16 keys, columns = the row's KM query heads (pre-scaled, columns
//     >= KM zero). Lane (col, h) owns the contiguous quarter [HS/4 h, HS/4 (h + 1)) of the head for
//     both operands, so K comes in as 16-byte LDS reads (ds_read_b128: 16 dims of one key), each
//     feeding two MFMAs (8 dims = one bf16x8 operand): HS / 32 MFMAs per 16 keys;
//   * one online-softmax step per tile and column over the lane's 16 scores + 2 shuffles;
//   * O^T += V^T . P^T per 32 keys: A = V^T from the row-major V tile with ds_read_b64_tr_b8 (the
//     8-bit transposed read: lane 2 q + p of a 16-lane group addresses bytes 8 p.. of key row q, lane
//     i receives dim i of the 8 rows; scripts/probe_tr8.hip prints the mapping), B = P^T straight
//     from the S^T accumulators.
//   * fp8 -> bf16: v_cvt_pk_f32_fp8 on each byte pair, then a pack of the two high halves (the low
//     16 bits of a widened e4m3 are zero): 8 VALU ops per 8-byte fragment.
// Key order. MFMA row m of 16-key subtile u is LDS row fkKey(u, m) = 32 (u >> 1) + 8 (m >> 2) +
// 4 (u & 1) + (m & 3): lane group h's S^T registers of subtiles 2 x, 2 x + 1 (MFMA rows 4 h .. 4 h + 3
// each) are then the 8 consecutive rows 32 x + 8 h .. + 7, in the order of P^T's 8 k-indices, which
// is what one transposed read of group h fetches.
//
// LDS image and banks. The DMA writes a wave-instruction lane-contiguously (lane l at byte 16 l), so
// rows are unpadded (HS bytes) and the swizzle is the choice of source piece: slot p of row r holds
// the row's 16-byte piece p ^ f(r). With r's bits r0..r5,
//   HS 128 (8 pieces): f = r1 | r3 << 1 | (r2 ^ r4) << 2      HS 64 (4 pieces): f = r3 | (r2 ^ r4) << 1.
// The 64 banks span 256 B = 2 (4) rows, so an access's bank group is (r0 [, r1], slot).
//   K read (ds_read_b128, 16 lanes per pass = one group h, all reading piece s): rows fkKey(u, col) =
//   32 x + 4 (u & 1) + 8 a + b (a = col >> 2, b = col & 3) vary r0 r1 = b, r3 r4 = a with r2, r5 fixed.
//   HS 128: quad 8 r0 + (s ^ f), f = (b1, a0, r2 ^ a1): (b0, b1, a0, a1) -> 16 distinct quads.
//   HS 64:  quad 4 (r0 r1) + (s ^ f), f = (a0, r2 ^ a1): again a bijection of (b, a): 16 quads.
//   V read (ds_read_b64_tr_b8, 32 lanes per pass = groups 2 y, 2 y + 1, all reading piece n): rows
//   32 x + 8 h + q (q = col >> 1) vary r0 r1 r2 = q, r3 = h0 with r4 = y, r5 fixed; lane half p = col & 1.
//   HS 128: 8-byte slot 16 r0 + 2 (n ^ f) + p, f = (q1, h0, q2 ^ y): (q0, q1, q2, h0, p) -> 32 slots.
//   HS 64:  slot 8 (r0 r1) + 2 (n ^ f) + p, f = (h0, q2 ^ y): 32 distinct slots.
// Kept from attn_mfma.hip: page ids loaded once per workgroup, one per lane, and shuffled to rows;
// LDS-DMA data ordered by a counted vmcnt followed by a workgroup barrier; keys past the chunk are
// masked, never branched around (the DMA re-reads the chunk's last key); no scratch.
#include "attn_prefill_dev.h"

namespace dl {
namespace hipk {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

static constexpr int kF8Threads = 256, kF8Waves = 4, kF8Tile = 64;
__host__ __device__ constexpr int f8TileBytes(int hs) { return kF8Tile * hs; }       // one K or V tile
__host__ __device__ constexpr int f8WaveBytes(int hs) { return 2 * 2 * f8TileBytes(hs); }  // 2 x (K + V)
__host__ __device__ constexpr size_t f8Lds(int hs) { return (size_t)kF8Waves * f8WaveBytes(hs) + 64; }
// bytes of the tail's LDS carve-up: oW, mW, lW, redL, mlL, flagL (attnFinish's scratch follows)
__host__ __device__ constexpr int f8MergeBytes(int km, int hs) {
    return 4 * (kF8Waves * km * hs + 2 * kF8Waves * km + km * hs + 2 * km + 4);
}

template <int HS>
__device__ __forceinline__ int f8Swz(int r) {
    if constexpr (HS == 128) return ((r >> 1) & 1) | (((r >> 3) & 1) << 1) | ((((r >> 2) ^ (r >> 4)) & 1) << 2);
    else return ((r >> 3) & 1) | ((((r >> 2) ^ (r >> 4)) & 1) << 1);
}
__device__ __forceinline__ int fkKey(int u, int m) { return 32 * (u >> 1) + 8 * (m >> 2) + 4 * (u & 1) + (m & 3); }

// 8 e4m3 bytes -> a bf16x8 MFMA operand (exact)
__device__ __forceinline__ bf16x8 fp8x8ToBf16(uint32_t w0, uint32_t w1) {
    auto pack = [](f32x2 v) { return (__float_as_uint(v.x) >> 16) | (__float_as_uint(v.y) & 0xffff0000u); };
    const u32x4 r = {pack(__builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false)), pack(__builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true)),
                     pack(__builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false)), pack(__builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true))};
    return __builtin_bit_cast(bf16x8, r);
}

template <int KM, int HS>
__global__ __launch_bounds__(kF8Threads) void attnDecodeFp8Kernel(AttnArgs a) {
    constexpr int TILE = kF8Tile, NU = TILE / 16, NH = TILE / 32, NT = HS / 16, DS = HS / 32, QD = HS / 4;
    constexpr int PPR = HS / 16, RPI = 1024 / HS, NI = TILE / RPI;  // pieces per row, rows and instructions per DMA'd tile
    constexpr int PPL = HS / 64;                                     // 16-byte K pieces per lane and key
    constexpr int TB = f8TileBytes(HS), WB = f8WaveBytes(HS);
    static_assert(2 * NI == HS / 8 && DS == 2 * PPL, "tile geometry");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, h = lane >> 4;
    const int pos = a.pos[b], sl = a.slot[b], len = pos + 1;
    int nSplit, ch;
    attnSplit(len, a.splitGrid, nSplit, ch, a.chunkMin, a.shortLen);
    if (c >= nSplit) return;
    const int t0 = c * ch, t1 = min(t0 + ch, len);
    const int nTiles = (t1 - t0 + TILE - 1) / TILE;
    // stamps stay in SGPRs until the end (a store would join the vmcnt accounting of the DMA)
    unsigned long long tr[6] = {a.trace ? wall_clock64() : 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};

    // this lane's column: query head g * KM + col (columns >= KM are zero and discarded), its quarter
    // QD h of the head; loaded first, waited for after the first two tiles' DMA is issued
    float4 qx[QD / 4];
    {
        const float *qp = a.q + (size_t)b * a.ldq + (size_t)(g * KM + min(col, KM - 1)) * HS + QD * h;
#pragma unroll
        for (int e = 0; e < QD / 4; e++) qx[e] = ld4(qp + 4 * e);
    }

    char *wbuf = smem + wave * WB;  // [2 buffers][K tile | V tile]
    const uint8_t *kc = reinterpret_cast<const uint8_t *>(a.kcache);
    const uint8_t *vc = reinterpret_cast<const uint8_t *>(a.vcache);
    const int nKv = a.kv0 / HS;
    // Paged cache: the chunk's page ids are loaded once, one per lane (a chunk spans at most 64
    // pages: attnFp8Refusal), and retired before any DMA; each key row's page is a lane shuffle.
    const KvMap &km = a.kvMap;
    const int pg0 = km.table ? t0 >> km.pageShift : 0;
    const bool pgLanes = km.table != nullptr;
    int pgReg = 0;
    if (pgLanes) {
        int v = km.table[sl * km.pagesPerSlot + pg0 + min(lane, ((t1 - 1) >> km.pageShift) - pg0)];
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(v));
        pgReg = v;
    }
    auto offOf = [&](int key) -> size_t {  // element (= byte) offset of head g's vector at this key
        if (!pgLanes) return kvOffAt(km, a.seqLen, nKv, HS, (size_t)sl, key, g);
        const int pg = __shfl(pgReg, (key >> km.pageShift) - pg0);
        return kvOffAt(km, a.seqLen, nKv, HS, (size_t)pg, key, g);
    };
    // DMA of tile i (keys t0 + 64 i ...) into buffer bf: NI + NI wave-instructions of RPI rows
    // (non-temporal: a decode row reads each layer's K / V once)
    auto issue = [&](int i, int bf) {
        char *kb = wbuf + bf * 2 * TB, *vb = kb + TB;
#pragma unroll
        for (int j = 0; j < NI; j++) {
            const int r = RPI * j + lane / PPR, p = lane % PPR;
            const int key = min(t0 + TILE * i + r, t1 - 1);  // past the chunk: masked below
            const size_t off = offOf(key) + (size_t)(p ^ f8Swz<HS>(r)) * 16;
            __builtin_amdgcn_global_load_lds(const_cast<uint8_t *>(kc + off),
                                             reinterpret_cast<__attribute__((address_space(3))) void *>(
                                                 reinterpret_cast<uintptr_t>(kb + j * 1024)), 16, 0, 2);
            __builtin_amdgcn_global_load_lds(const_cast<uint8_t *>(vc + off),
                                             reinterpret_cast<__attribute__((address_space(3))) void *>(
                                                 reinterpret_cast<uintptr_t>(vb + j * 1024)), 16, 0, 2);
        }
    };

    f32x4 o[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;
    const int nRounds = (nTiles + kF8Waves - 1) / kF8Waves;
    // both prologue tiles are issued unconditionally (a tile past the chunk re-reads its last key:
    // harmless, never consumed), so the vmcnt the q values wait for is the same on every wave
    issue(wave, 0);
    issue(wave + kF8Waves, 1);
    const float qs = col < KM ? 1.0f / sqrtf((float)HS) : 0.f;
    bf16x8 qf[DS];  // qf[s]: dims QD h + 8 s .. + 7
#pragma unroll
    for (int s = 0; s < DS; s++) {
        const float4 x0 = qx[2 * s], x1 = qx[2 * s + 1];
        const float v[8] = {x0.x * qs, x0.y * qs, x0.z * qs, x0.w * qs, x1.x * qs, x1.y * qs, x1.z * qs, x1.w * qs};
#pragma unroll
        for (int j = 0; j < 8; j++) qf[s][j] = (__bf16)v[j];
    }
    // LDS byte offsets of this lane's reads inside a tile (the same for every tile); V: lane 2 q + p
    // of group h addresses row 32 x + 8 h + q, bytes 8 p.. of piece n
    const int vRow = 8 * h + (col >> 1), vHalf = 8 * (col & 1);
    if (a.trace) tr[1] = wall_clock64();
    for (int k = 0; k < nRounds; k++) {
        const int i = k * kF8Waves + wave;
        if (i + kF8Waves < nTiles) {  // tile i landed, tile i + 4 in flight
            if constexpr (HS == 128) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        if (a.trace && k == 0) tr[2] = wall_clock64();
        if (i >= nTiles) continue;  // wave-uniform; the barrier above is reached by every wave
        const char *kb = wbuf + (k & 1) * 2 * TB, *vb = kb + TB;
        const int tb = t0 + TILE * i;
        f32x4 st[NU];
#pragma unroll
        for (int u = 0; u < NU; u++) {
            st[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int r = fkKey(u, col);
#pragma unroll
            for (int e = 0; e < PPL; e++) {
                const u32x4 kw = *reinterpret_cast<const u32x4 *>(kb + r * HS + 16 * ((PPL * h + e) ^ f8Swz<HS>(r)));
                st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8ToBf16(kw.x, kw.y), qf[2 * e], st[u], 0, 0, 0);
                st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8ToBf16(kw.z, kw.w), qf[2 * e + 1], st[u], 0, 0, 0);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < NU; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (tb + fkKey(u, 4 * h + e) >= t1) st[u][e] = -INFINITY;
                mx = fmaxf(mx, st[u][e]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);
        const float corr = m == -INFINITY ? 0.f : __expf(m - mn);
        bf16x8 pf[NH];  // pf[x][4 (u & 1) + e]: key 32 x + 8 h + 4 (u & 1) + e
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < NU; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float p = st[u][e] == -INFINITY ? 0.f : __expf(st[u][e] - mn);
                ps += p;
                pf[u >> 1][4 * (u & 1) + e] = (__bf16)p;
            }
        lsum = lsum * corr + ps;
        m = mn;
#pragma unroll
        for (int n = 0; n < NT; n++) {
            o[n] *= corr;
#pragma unroll
            for (int x = 0; x < NH; x++) {
                const int r = 32 * x + vRow;
                const char *ad = vb + r * HS + 16 * (n ^ f8Swz<HS>(r)) + vHalf;
                const i32x2 vw = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
                    reinterpret_cast<__attribute__((address_space(3))) i32x2 *>(reinterpret_cast<uintptr_t>(ad)));
                o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8ToBf16((uint32_t)vw.x, (uint32_t)vw.y), pf[x], o[n], 0, 0, 0);
            }
        }
        // this buffer's reads retire before the DMA of tile i + 8 overwrites it
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (i + 2 * kF8Waves < nTiles) issue(i + 2 * kF8Waves, k & 1);
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (a.trace) tr[3] = wall_clock64();

    // merge the waves (LDS: the tile buffers are free once every wave is past its loop)
    __syncthreads();
    float *oW = reinterpret_cast<float *>(smem);  // [4 waves][KM][HS]
    float *mW = oW + kF8Waves * KM * HS;          // [4][KM]
    float *lW = mW + kF8Waves * KM;               // [4][KM]
    float *redL = lW + kF8Waves * KM;             // [KM][HS]
    float *mlL = redL + KM * HS;                  // [KM][2]
    int *flagL = reinterpret_cast<int *>(mlL + 2 * KM);
    float *scratch = reinterpret_cast<float *>(flagL + 4);  // attnFinish: 2 * KM * splitGrid
    if (col < KM) {
        if (h == 0) {
            mW[wave * KM + col] = wave < nTiles ? m : -INFINITY;
            lW[wave * KM + col] = wave < nTiles ? lsum : 0.f;
        }
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int e = 0; e < 4; e++) oW[(wave * KM + col) * HS + 16 * n + 4 * h + e] = o[n][e];
    }
    __syncthreads();
    for (int i = tid; i < KM * HS; i += kF8Threads) {
        const int hh = i / HS;
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < kF8Waves; w++) M = fmaxf(M, mW[w * KM + hh]);
        float acc = 0.f, Ls = 0.f;
#pragma unroll
        for (int w = 0; w < kF8Waves; w++) {
            const float e = mW[w * KM + hh] == -INFINITY ? 0.f : __expf(mW[w * KM + hh] - M);
            acc += e * oW[(w * KM + hh) * HS + (i % HS)];
            Ls += e * lW[w * KM + hh];
        }
        redL[i] = acc;
        if (i % HS == 0) {
            mlL[hh * 2] = M;
            mlL[hh * 2 + 1] = Ls;
        }
    }
    __syncthreads();
    if (a.trace) tr[4] = wall_clock64();
    const bool fin = attnFinish<KM, HS, kF8Threads>(a, b, g, c, nSplit, redL, mlL, flagL, scratch);
    if (a.trace && tid == 0) {
        tr[5] = wall_clock64();
        unsigned long long *t = a.trace + 8 * (((size_t)b * gridDim.y + c) * gridDim.x + g);
        for (int i = 0; i < 6; i++) t[i] = tr[i];
        t[6] = fin ? 1ull : 0ull;
    }
}

// ------------------------------------------------------------------------------------------------
// Prefill attention over fp8 caches: the prompt rows of a batched forward. Semantics are the decode
// kernel's (bytes widened to bf16 in registers, Q . scale and P rounded to bf16,
// v_mfma_f32_16x16x32_bf16, f32 online softmax, no scale factor); the work split is the other prefill
// kernels' (attn_prefill.hip, attn_mfma.hip): one workgroup owns one KV head and a block of 4 x 16 / KM
// consecutive rows of one slot, a wave's 16 MFMA columns are (row, query head) pairs, all four waves
// read every K / V tile of the chunk from LDS, long contexts split over grid.y by attnPrefillSplit and
// finish through pfFinish. The decode kernel walked the context once per row: a 64-row chunk at
// position p read 64 x p keys, here it reads p per row block.
//
// Tiles and LDS image are the decode kernel's: 64-key tiles of unpadded HS-byte rows, f8Swz source
// pieces, fkKey key order, K by ds_read_b128 (two MFMAs each), V^T by ds_read_b64_tr_b8. Neither
// fkKey nor f8Swz reads row bit 5, so a tile is two independent 32-key halves with the same bank
// maps, and the half is the unit of everything that attnPrefillSplit's 32-key granularity touches:
//   * a chunk starts at a multiple of 32, so a 64-key tile may straddle a page of a paged cache; a
//     half never does. The page list (LDS, filled before any DMA) has one entry per half;
//   * the DMA unit is the half: wave w copies half w of a round (K and V: HS / 32 + HS / 32
//     wave-instructions of 1024 / HS rows), so a round is 4 halves = 2 tiles = 128 keys;
//   * a chunk's last tile may own one half only. The other half is still copied (its keys clamp to
//     the chunk's last key, as every row past the chunk does), because its V bytes enter the O^T MFMA
//     with P = 0 and stale LDS could hold NaN codes.
// Staging is attnPrefillDmaKernel's: rounds copied by LDS-DMA two ahead, a counted vmcnt (this wave's
// copy of the round landed, the next round's may stay in flight), a workgroup barrier, every wave
// consumes both tiles, a second barrier frees the buffer for round r + 2.
//
// What the halved bytes are spent on. Two rounds of 128 keys in flight are the bf16 kernel's keys in
// flight (it holds 2 x 4 tiles of 32) in half its LDS: 64 KB at head size 128 (32 KB at 64) instead of
// 128 KB, so two (four) workgroups share a CU where the bf16 kernel runs one. The alternatives were
// twice the keys in flight per workgroup (four 64-key tiles a round) or a third round at the same
// 128 KB. Per tile and wave this kernel issues 32 MFMAs but also 256 VALU conversions (8 per 8-byte
// fragment, every wave converting the tiles for its own columns) before the softmax's VALU work, so a
// lone workgroup leaves the CU idle at both barriers of a round and whenever its four waves sit in
// the same conversion or exp stretch; deeper staging would only lengthen a queue that the DMA already
// keeps full, while a second resident workgroup runs its MFMAs and conversions in those gaps. The
// cost is none in keys in flight per CU (2 x 256 = the bf16 kernel's 512 at HS 128).
// No non-temporal hint on the DMA (every row block of the prompt reads the same tiles); no scratch.
// ------------------------------------------------------------------------------------------------
static constexpr int kFpRound = 2;       // 64-key tiles per round (4 halves, one per wave)
static constexpr int kFpMaxHalves = 256; // per-chunk page list (paged caches): one page per 32-key half
__host__ __device__ constexpr size_t fpLds(int hs) { return (size_t)2 * kFpRound * 2 * f8TileBytes(hs) + 64; }

template <int KM, int HS>
__global__ __launch_bounds__(kF8Threads) void attnPrefillFp8Kernel(AttnArgs a, int nRows) {
    constexpr int TILE = kF8Tile, HALF = TILE / 2, NU = TILE / 16, NH = TILE / 32, NT = HS / 16, DS = HS / 32, QD = HS / 4;
    constexpr int PPR = HS / 16, RPI = 1024 / HS, NIH = HALF / RPI;  // pieces per row, rows per DMA instruction, instructions per half
    constexpr int PPL = HS / 64;                                      // 16-byte K pieces per lane and key
    constexpr int TB = f8TileBytes(HS), RPW = 16 / KM, RPB = kF8Waves * RPW;
    static_assert(kF8Threads == kPfThreads && kF8Waves == kPfWaves && 2 * kFpRound == kF8Waves, "pfFinish's workgroup, one half per wave");
    static_assert(HALF == kAttnPrefillTile && DS == 2 * PPL, "tile geometry");
    static_assert(2 * kFpRound * 2 * TB >= 4 * (64 * (HS / 2) + 64), "combine weights must fit the tiles");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int pageL[kFpMaxHalves];
    const int nKv = a.nHeads0 / KM;
    const int g = blockIdx.x % nKv, rb = blockIdx.x / nKv, c = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, h = lane >> 4;
    const int b0 = rb * RPB;
    const int maxLen = rowsMaxLen(a.pos, b0, RPB, nRows);
    int nSplit, ch;
    attnPrefillSplit(maxLen, a.splitGrid, HS, kAttnPrefillChunk, nSplit, ch);
    if (c >= nSplit) return;
    const int k0 = c * ch, k1 = min(k0 + ch, maxLen);
    const int sl = a.slot[b0];  // every row of the block (host-checked)
    // this lane's column: a (row, query head) pair; its quarter QD h of the head for S^T
    const int row = b0 + wave * RPW + col / KM, head = g * KM + col % KM;
    const bool rowOk = row < nRows;
    const int myLen = rowOk ? a.pos[row] + 1 : 0;
    const float scale = 1.0f / sqrtf((float)HS);
    bf16x8 qf[DS];  // qf[s]: dims QD h + 8 s .. + 7
#pragma unroll
    for (int s = 0; s < DS; s++) {
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (rowOk) {
            const float *qp = a.q + (size_t)row * a.ldq + (size_t)head * HS + QD * h + 8 * s;
            const float4 x0 = ld4(qp), x1 = ld4(qp + 4);
            v[0] = x0.x * scale; v[1] = x0.y * scale; v[2] = x0.z * scale; v[3] = x0.w * scale;
            v[4] = x1.x * scale; v[5] = x1.y * scale; v[6] = x1.z * scale; v[7] = x1.w * scale;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) qf[s][j] = (__bf16)v[j];
    }
    const uint8_t *kc = reinterpret_cast<const uint8_t *>(a.kcache);
    const uint8_t *vc = reinterpret_cast<const uint8_t *>(a.vcache);
    const int nHalves = (k1 - k0 + HALF - 1) / HALF, nTiles = (nHalves + 1) / 2;
    const int nRounds = (nTiles + kFpRound - 1) / kFpRound;
    // paged cache: the chunk's per-half pages in LDS before any DMA (a table load per key row would
    // put a vmcnt(0) drain before every DMA pair, contiguous caches included)
    if (a.kvMap.table)
        for (int i = tid; i < nHalves; i += kF8Threads) pageL[i] = (int)kvPageOf(a.kvMap, sl, k0 + i * HALF);
    __syncthreads();
    auto tileBuf = [&](int bf, int tt) { return smem + (size_t)(bf * kFpRound + tt) * 2 * TB; };
    // wave w copies half w of round r (half w & 1 of tile w >> 1) into buffer bf: NIH + NIH
    // wave-instructions, or none when the tile is past the chunk
    auto issue = [&](int r, int bf) {
        const int hf = 2 * kFpRound * r + wave;
        if ((hf >> 1) >= nTiles) return;
        char *kb = tileBuf(bf, wave >> 1) + (wave & 1) * HALF * HS, *vb = kb + TB;
        const size_t blk = a.kvMap.table ? (size_t)pageL[min(hf, nHalves - 1)] : (size_t)sl;
#pragma unroll
        for (int j = 0; j < NIH; j++) {
            const int rr = RPI * j + lane / PPR, p = lane % PPR;
            const int key = min(k0 + HALF * hf + rr, k1 - 1);  // past the chunk: masked below (in half nHalves - 1)
            const size_t off = kvOffAt(a.kvMap, a.seqLen, nKv, HS, blk, key, g) + (size_t)(p ^ f8Swz<HS>(rr)) * 16;
            __builtin_amdgcn_global_load_lds(const_cast<uint8_t *>(kc + off),
                                             reinterpret_cast<__attribute__((address_space(3))) void *>(
                                                 reinterpret_cast<uintptr_t>(kb + j * 1024)), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(const_cast<uint8_t *>(vc + off),
                                             reinterpret_cast<__attribute__((address_space(3))) void *>(
                                                 reinterpret_cast<uintptr_t>(vb + j * 1024)), 16, 0, 0);
        }
    };
    f32x4 o[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;
    // V: lane 2 q + p of group h addresses row 32 x + 8 h + q, bytes 8 p.. of piece n
    const int vRow = 8 * h + (col >> 1), vHalf = 8 * (col & 1);
    issue(0, 0);
    if (nRounds > 1) issue(1, 1);
    for (int r = 0; r < nRounds; r++) {
        // this wave's copy of round r landed (round r + 1's may stay in flight), then every wave's
        if (r + 1 < nRounds && ((2 * kFpRound * (r + 1) + wave) >> 1) < nTiles) {
            if constexpr (HS == 128) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        for (int tt = 0; tt < kFpRound; tt++) {
            const int t = kFpRound * r + tt;
            if (t >= nTiles) break;  // uniform over the workgroup
            const char *kb = tileBuf(r & 1, tt), *vb = kb + TB;
            const int tb = k0 + TILE * t;
            f32x4 st[NU];
#pragma unroll
            for (int u = 0; u < NU; u++) {
                st[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                const int rr = fkKey(u, col);
#pragma unroll
                for (int e = 0; e < PPL; e++) {
                    const u32x4 kw = *reinterpret_cast<const u32x4 *>(kb + rr * HS + 16 * ((PPL * h + e) ^ f8Swz<HS>(rr)));
                    st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8ToBf16(kw.x, kw.y), qf[2 * e], st[u], 0, 0, 0);
                    st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8ToBf16(kw.z, kw.w), qf[2 * e + 1], st[u], 0, 0, 0);
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int u = 0; u < NU; u++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int key = tb + fkKey(u, 4 * h + e);
                    if (key >= k1 || key >= myLen) st[u][e] = -INFINITY;
                    mx = fmaxf(mx, st[u][e]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m, mx);
            const float corr = m == -INFINITY ? 0.f : __expf(m - mn);
            bf16x8 pf[NH];  // pf[x][4 (u & 1) + e]: key 32 x + 8 h + 4 (u & 1) + e
            float ps = 0.f;
#pragma unroll
            for (int u = 0; u < NU; u++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float p = st[u][e] == -INFINITY ? 0.f : __expf(st[u][e] - mn);
                    ps += p;
                    pf[u >> 1][4 * (u & 1) + e] = (__bf16)p;
                }
            lsum = lsum * corr + ps;
            m = mn;
#pragma unroll
            for (int n = 0; n < NT; n++) {
                o[n] *= corr;
#pragma unroll
                for (int x = 0; x < NH; x++) {
                    const int rr = 32 * x + vRow;
                    const char *ad = vb + rr * HS + 16 * (n ^ f8Swz<HS>(rr)) + vHalf;
                    const i32x2 vw = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
                        reinterpret_cast<__attribute__((address_space(3))) i32x2 *>(reinterpret_cast<uintptr_t>(ad)));
                    o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8ToBf16((uint32_t)vw.x, (uint32_t)vw.y), pf[x], o[n], 0, 0, 0);
                }
            }
        }
        // every wave's reads of buffer r & 1 retired before round r + 2 is copied into it
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (r + 2 < nRounds) issue(r + 2, r & 1);
    }
    // wts [64 columns][nSplit <= HS / 2] and tot [64] reuse the tiles; the flag sits behind them
    float *wts = reinterpret_cast<float *>(smem);
    pfFinish<HS>(a, nRows, o, m, lsum, nSplit, rb, g, c, b0, row, head, wts, wts + 64 * (HS / 2),
                 *reinterpret_cast<int *>(smem + 2 * kFpRound * 2 * TB));
}

bool attnFp8Supported(const AttnArgs &a) {
    return a.kvFp8 && (a.hs == 128 || a.hs == 64) && (a.kvMul == 1 || a.kvMul == 2 || a.kvMul == 4 || a.kvMul == 8) &&
           a.nHeads0 % a.kvMul == 0;
}

const char *attnFp8Refusal(const AttnArgs &a) {
    if (!attnFp8Supported(a))
        return "launchAttentionFp8: fp8 KV caches need head size 64 or 128 and kvMul 1, 2, 4 or 8";
    // the tail's carve-up (wave merge, combine flags) and attnFinish's scratch share the tile buffers
    if ((size_t)f8MergeBytes(a.kvMul, a.hs) + (size_t)2 * a.kvMul * a.splitGrid * 4 > f8Lds(a.hs))
        return "launchAttentionFp8: attention split grid too large";
    if (a.kvMap.table && (a.chunkMax >> a.kvMap.pageShift) + 2 > 64)
        return "launchAttentionFp8: a chunk spans more than 64 pages (one page id per lane)";
    return nullptr;
}

std::string attnFp8KernelName(const AttnArgs &a) {
    return "attnDecodeFp8Kernel<" + std::to_string(a.kvMul) + "," + std::to_string(a.hs) + ">";
}

// preloadModules(): one kernel of this translation unit's code object
const void *attnFp8ModuleKernel() { return (const void *)attnDecodeFp8Kernel<4, 128>; }

void launchAttentionFp8(const AttnArgs &a, int B, hipStream_t s) {
    if (const char *why = attnFp8Refusal(a)) throw Error(why);
    const dim3 grid(a.nHeads0 / a.kvMul, a.splitGrid, B);
#define DL_F8_CASE(K, H)                                                                               \
    if (a.kvMul == K && a.hs == H) {                                                                   \
        allowLds((const void *)attnDecodeFp8Kernel<K, H>, f8Lds(H));                                   \
        hipLaunchKernelGGL((attnDecodeFp8Kernel<K, H>), grid, dim3(kF8Threads), f8Lds(H), s, a);       \
        return;                                                                                        \
    }
    DL_F8_CASE(1, 128) DL_F8_CASE(2, 128) DL_F8_CASE(4, 128) DL_F8_CASE(8, 128)
    DL_F8_CASE(1, 64) DL_F8_CASE(2, 64) DL_F8_CASE(4, 64) DL_F8_CASE(8, 64)
#undef DL_F8_CASE
    throw Error("launchAttentionFp8: fp8 KV caches need head size 64 or 128 and kvMul 1, 2, 4 or 8");
}

const char *attnPrefillFp8Refusal(const AttnArgs &a) {
    if (!attnFp8Supported(a))
        return "launchAttentionPrefillFp8: fp8 KV caches need head size 64 or 128 and kvMul 1, 2, 4 or 8";
    // the combine's weights (64 columns x up to hs / 2 splits) and totals live in the tile buffers
    const int maxSplits = std::max(1, std::min(a.splitGrid, a.hs / 2));
    if ((size_t)4 * (64 * maxSplits + 64) + 64 > fpLds(a.hs))
        return "launchAttentionPrefillFp8: attention split grid too large";
    // the longest chunk's 32-key halves fit the kernel's LDS page list
    if (a.kvMap.table && ((a.seqLen + maxSplits - 1) / maxSplits + kAttnPrefillTile - 1) / kAttnPrefillTile + 1 > kFpMaxHalves)
        return "launchAttentionPrefillFp8: paged context too long for the per-chunk page list";
    return nullptr;
}

std::string attnPrefillFp8KernelName(const AttnArgs &a) {
    return "attnPrefillFp8Kernel<" + std::to_string(a.kvMul) + "," + std::to_string(a.hs) + ">";
}

void launchAttentionPrefillFp8(const AttnArgs &a, int nRows, hipStream_t s) {
    if (const char *why = attnPrefillFp8Refusal(a)) throw Error(why);
    const int nKv = a.nHeads0 / a.kvMul, rpb = kF8Waves * (16 / a.kvMul);
    const dim3 grid(nKv * ((nRows + rpb - 1) / rpb), a.splitGrid);
#define DL_FP_CASE(K, H)                                                                                      \
    if (a.kvMul == K && a.hs == H) {                                                                          \
        allowLds((const void *)attnPrefillFp8Kernel<K, H>, fpLds(H));                                         \
        hipLaunchKernelGGL((attnPrefillFp8Kernel<K, H>), grid, dim3(kF8Threads), fpLds(H), s, a, nRows);      \
        return;                                                                                               \
    }
    DL_FP_CASE(1, 128) DL_FP_CASE(2, 128) DL_FP_CASE(4, 128) DL_FP_CASE(8, 128)
    DL_FP_CASE(1, 64) DL_FP_CASE(2, 64) DL_FP_CASE(4, 64) DL_FP_CASE(8, 64)
#undef DL_FP_CASE
    throw Error("launchAttentionPrefillFp8: fp8 KV caches need head size 64 or 128 and kvMul 1, 2, 4 or 8");
}

}  // namespace hipk
}  // namespace dl
