// Decode attention on MFMA for f32 KV caches (the default --kv-dtype): the schedule of
// attnDecodeMfmaKernel (attn_mfma.hip) on v_mfma_f32_16x16x4_f32, K and V read unrounded, so the
// result differs from the VALU kernel (attnTask) by f32 reassociation only.
//
// One workgroup owns one (row, KV head, key chunk), grid (nKvHeads, splitGrid, B), 256 threads; its
// 4 waves split the chunk's tiles round-robin (wave w: tiles w, w + 4, ...). An f32 key row is 4 HS
// bytes, so a tile is 16 keys at head size 128 and 32 keys at head size 64: 8 KB per K or V tile
// either way, 2 buffers x (K + V) x 4 waves = 128 KB of LDS, the bf16 kernel's budget, and a tile is
// 8 + 8 wave-wide LDS-DMA instructions of 1 KB (2 or 4 key rows each), so the counted waits carry
// over: vmcnt(16) with the next tile in flight, vmcnt(0) without, then a workgroup barrier before
// the first ds_read of the buffer (every wave runs the same number of rounds). Per tile a wave
//   * S^T = K . Q^T: A = 16 keys x 4 dims from the LDS K tile, B = the row's KM query heads as the
//     MFMA columns (pre-scaled by 1 / sqrt(HS), columns >= KM zero). Lane (col, h) holds A[col][h] and
//     B[h][col]; lane group h owns the contiguous quarter [QD h, QD h + QD) of the head (QD = HS / 4),
//     so MFMA e multiplies K[key 16 u + col][QD h + e] by Q[col][QD h + e] and K is read in 16-byte
//     LDS reads: HS / 4 MFMAs per 16 keys.
//   * one online-softmax step per tile and column: the lane holds S[key 16 u + 4 h + i][col], so the
//     max and the sum take the lane's 4 (or 8) scores and two cross-lane shuffles; P stays f32.
//   * O^T += V^T . P^T: MFMA (u, i, n) multiplies V[key 16 u + 4 h + i][dim 16 n + col] (a 4-byte
//     read of the row-major V tile: 16 consecutive lanes read 16 consecutive dims of one key) by
//     P[key 16 u + 4 h + i][col], the S^T accumulator the lane already holds: HS / 16 x 4 MFMAs per
//     16 keys and P never moves.
// The 4 waves' (max, sum, O) merge in LDS and chunks combine through attnFinish with the attnSplit
// plan, as in the VALU and bf16 kernels (same partial buffers, output formats, stamps, counters).
//
// LDS image. The DMA lays a wave instruction out lane-contiguously (lane l at byte 16 l), so rows
// are unpadded (512 B / 256 B) and the swizzle is the choice of source piece: slot p of key row r
// holds the row's 16-byte piece p ^ (r & 15), i.e. piece s of row r lives at 16 (s ^ (r & 15)).
// XOR with a 4-bit value keeps a piece in its 256-B half of a 512-B row, and the 64 banks (256 B)
// see only the low 4 bits of the slot.
//   K read (ds_read_b128, 16 lanes cover the 64 banks): the 16 lanes of a group h read the same
//   piece s of rows 16 u + col, col = 0..15: slots s ^ col, 16 distinct bank quads.
//   V read (ds_read_b32, 64 lanes cover the 64 banks): lane (col, h) reads word col & 3 of piece
//   4 n + (col >> 2) of row 16 u + 4 h + i: slot (4 n + (col >> 2)) ^ (4 h + i) = 4 (n ^ h) +
//   ((col >> 2) ^ i) (mod 16), distinct over the 16 (h, col >> 2) pairs, times the 4 words of a
//   piece: 64 distinct banks.
#include "decode_dev.h"

namespace dl {
namespace hipk {

static constexpr int kAfThreads = 256, kAfWaves = 4;
static constexpr int kAfTileBytes = 8192;                  // one K or V tile: 16 keys x 512 B / 32 keys x 256 B
static constexpr int kAfWaveBytes = 2 * 2 * kAfTileBytes;  // double-buffered K + V per wave
static constexpr size_t kAfLds = (size_t)kAfWaves * kAfWaveBytes + 64;
// bytes of the tail's LDS carve-up below: oW, mW, lW, redL, mlL, flagL (attnFinish's scratch follows)
__host__ __device__ constexpr int afMergeBytes(int km, int hs) {
    return 4 * (kAfWaves * km * hs + 2 * kAfWaves * km + km * hs + 2 * km + 4);
}

template <int KM, int HS>
__global__ __launch_bounds__(kAfThreads) void attnDecodeF32MfmaKernel(AttnArgs a) {
    constexpr int TILE = kAfTileBytes / (4 * HS);  // keys per tile: 16 (HS 128) / 32 (HS 64)
    constexpr int NU = TILE / 16, NT = HS / 16, QD = HS / 4;
    constexpr int RB = 4 * HS, PPR = HS / 4, RPI = 1024 / RB;  // row bytes, 16-B pieces per row, rows per DMA
    static_assert(TILE * RB == kAfTileBytes && TILE / RPI == 8, "a tile is 8 DMA instructions");
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

    // this lane's column: query head g * KM + col (columns >= KM are zero and discarded), its
    // quarter QD h of the head; loaded first, waited for after the first two tiles' DMA is issued
    float4 qx[QD / 4];
    {
        const float *qp = a.q + (size_t)b * a.ldq + (size_t)(g * KM + min(col, KM - 1)) * HS + QD * h;
#pragma unroll
        for (int e = 0; e < QD / 4; e++) qx[e] = ld4(qp + 4 * e);
    }

    char *wbuf = smem + wave * kAfWaveBytes;  // [2 buffers][K tile | V tile]
    const float *kc = reinterpret_cast<const float *>(a.kcache);
    const float *vc = reinterpret_cast<const float *>(a.vcache);
    const int nKv = a.kv0 / HS;
    // Paged cache: the chunk's page ids are loaded once, one per lane (a chunk spans at most 64
    // pages: attnF32MfmaRefusal), and retired before any DMA; each key row's page is a lane shuffle.
    const KvMap &km = a.kvMap;
    const int pg0 = km.table ? t0 >> km.pageShift : 0;
    const bool pgLanes = km.table != nullptr;
    int pgReg = 0;
    if (pgLanes) {
        int v = km.table[sl * km.pagesPerSlot + pg0 + min(lane, ((t1 - 1) >> km.pageShift) - pg0)];
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(v));
        pgReg = v;
    }
    auto offOf = [&](int key) -> size_t {  // element offset of head g's vector at this key
        if (!pgLanes) return kvOffAt(km, a.seqLen, nKv, HS, (size_t)sl, key, g);
        const int pg = __shfl(pgReg, (key >> km.pageShift) - pg0);
        return kvOffAt(km, a.seqLen, nKv, HS, (size_t)pg, key, g);
    };
    // DMA of tile i (keys t0 + TILE i ...) into buffer bf: 8 + 8 wave-instructions of RPI rows
    // (non-temporal: a decode row reads each layer's K / V once)
    auto issue = [&](int i, int bf) {
        char *kb = wbuf + bf * 2 * kAfTileBytes, *vb = kb + kAfTileBytes;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int r = RPI * j + lane / PPR, p = lane % PPR;
            const int key = min(t0 + TILE * i + r, t1 - 1);  // past the chunk: masked below
            const size_t off = offOf(key) + (size_t)(p ^ (r & 15)) * 4;
            __builtin_amdgcn_global_load_lds(const_cast<float *>(kc + off),
                                             reinterpret_cast<__attribute__((address_space(3))) void *>(
                                                 reinterpret_cast<uintptr_t>(kb + j * 1024)), 16, 0, 2);
            __builtin_amdgcn_global_load_lds(const_cast<float *>(vc + off),
                                             reinterpret_cast<__attribute__((address_space(3))) void *>(
                                                 reinterpret_cast<uintptr_t>(vb + j * 1024)), 16, 0, 2);
        }
    };

    f32x4 o[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;
    const int nRounds = (nTiles + kAfWaves - 1) / kAfWaves;
    // both prologue tiles are issued unconditionally (a tile past the chunk re-reads its last key:
    // harmless, never consumed), so the vmcnt the q values wait for is the same on every wave
    issue(wave, 0);
    issue(wave + kAfWaves, 1);
    const float qs = col < KM ? 1.0f / sqrtf((float)HS) : 0.f;
    float q[QD];
#pragma unroll
    for (int e = 0; e < QD / 4; e++) {
        q[4 * e] = qx[e].x * qs;
        q[4 * e + 1] = qx[e].y * qs;
        q[4 * e + 2] = qx[e].z * qs;
        q[4 * e + 3] = qx[e].w * qs;
    }
    // LDS byte offsets of this lane's reads inside a tile (the same for every tile):
    // K: row 16 u + col, pieces (QD / 4) h + e4 -> slot ^ col; V: see the header comment
    const int kOff = col * RB, kPiece = (QD / 4) * h;
    const int vOff = 4 * h * RB + 4 * (col & 3), c4 = col >> 2;
    if (a.trace) tr[1] = wall_clock64();
    for (int k = 0; k < nRounds; k++) {
        const int i = k * kAfWaves + wave;
        if (i + kAfWaves < nTiles)
            asm volatile("s_waitcnt vmcnt(16)" ::: "memory");  // tile i landed, tile i + 4 in flight
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (a.trace && k == 0) tr[2] = wall_clock64();
        if (i >= nTiles) continue;  // wave-uniform; the barrier above is reached by every wave
        const char *kb = wbuf + (k & 1) * 2 * kAfTileBytes, *vb = kb + kAfTileBytes;
        const int tb = t0 + TILE * i;
        f32x4 st[NU], sx[NU];  // two accumulator chains per subtile (even / odd pieces), summed below
#pragma unroll
        for (int u = 0; u < NU; u++) st[u] = sx[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e4 = 0; e4 < QD / 4; e4++) {
#pragma unroll
            for (int u = 0; u < NU; u++) {
                const f32x4 kf = *reinterpret_cast<const f32x4 *>(kb + 16 * u * RB + kOff + 16 * ((kPiece + e4) ^ col));
                f32x4 &acc = e4 & 1 ? sx[u] : st[u];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j], q[4 * e4 + j], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < NU; u++) st[u] += sx[u];
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < NU; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (tb + 16 * u + 4 * h + e >= t1) st[u][e] = -INFINITY;
                mx = fmaxf(mx, st[u][e]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);
        const float corr = m == -INFINITY ? 0.f : __expf(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < NU; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                st[u][e] = st[u][e] == -INFINITY ? 0.f : __expf(st[u][e] - mn);  // P, in place
                ps += st[u][e];
            }
        lsum = lsum * corr + ps;
        m = mn;
#pragma unroll
        for (int n = 0; n < NT; n++) o[n] *= corr;
#pragma unroll
        for (int u = 0; u < NU; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                // row 16 u + 4 h + e (r & 15 = 4 h + e), piece 4 n + c4 -> slot 4 (n ^ h) + (c4 ^ e) (+ 16)
                const char *vrow = vb + (16 * u + e) * RB + vOff + 16 * (c4 ^ e);
#pragma unroll
                for (int n = 0; n < NT; n++) {
                    const float vf = *reinterpret_cast<const float *>(vrow + 64 * ((n & 3) ^ h) + 256 * (n >> 2));
                    o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf, st[u][e], o[n], 0, 0, 0);
                }
            }
        // this buffer's reads retire before the DMA of tile i + 8 overwrites it
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (i + 2 * kAfWaves < nTiles) issue(i + 2 * kAfWaves, k & 1);
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (a.trace) tr[3] = wall_clock64();

    // merge the waves (LDS: the tile buffers are free once every wave is past its loop)
    __syncthreads();
    float *oW = reinterpret_cast<float *>(smem);  // [4 waves][KM][HS]
    float *mW = oW + kAfWaves * KM * HS;          // [4][KM]
    float *lW = mW + kAfWaves * KM;               // [4][KM]
    float *redL = lW + kAfWaves * KM;             // [KM][HS]
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
    for (int i = tid; i < KM * HS; i += kAfThreads) {
        const int hh = i / HS;
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < kAfWaves; w++) M = fmaxf(M, mW[w * KM + hh]);
        float acc = 0.f, Ls = 0.f;
#pragma unroll
        for (int w = 0; w < kAfWaves; w++) {
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
    const bool fin = attnFinish<KM, HS, kAfThreads>(a, b, g, c, nSplit, redL, mlL, flagL, scratch);
    if (a.trace && tid == 0) {
        tr[5] = wall_clock64();
        unsigned long long *t = a.trace + 8 * (((size_t)b * gridDim.y + c) * gridDim.x + g);
        for (int i = 0; i < 6; i++) t[i] = tr[i];
        t[6] = fin ? 1ull : 0ull;
    }
}

bool attnF32MfmaSupported(const AttnArgs &a) {
    return !a.kvBf16 && (a.hs == 128 || a.hs == 64) && (a.kvMul == 1 || a.kvMul == 2 || a.kvMul == 4 || a.kvMul == 8) &&
           a.nHeads0 % a.kvMul == 0;
}

const char *attnF32MfmaRefusal(const AttnArgs &a) {
    if (!attnF32MfmaSupported(a)) return "launchAttentionMfma: unsupported head size or kvMul (f32 cache)";
    // the tail's carve-up (wave merge, combine flags) and attnFinish's scratch share the tile buffers
    if ((size_t)afMergeBytes(a.kvMul, a.hs) + (size_t)2 * a.kvMul * a.splitGrid * 4 > kAfLds)
        return "launchAttentionMfma: attention split grid too large (f32 cache)";
    if (a.kvMap.table && (a.chunkMax >> a.kvMap.pageShift) + 2 > 64)
        return "launchAttentionMfma: a chunk spans more than 64 pages (one page id per lane)";
    return nullptr;
}

// preloadModules(): one kernel of this translation unit's code object
const void *attnF32MfmaModuleKernel() { return (const void *)attnDecodeF32MfmaKernel<4, 128>; }

void launchAttentionF32Mfma(const AttnArgs &a, int B, hipStream_t s) {
    const dim3 grid(a.nHeads0 / a.kvMul, a.splitGrid, B);
    if (const char *why = attnF32MfmaRefusal(a)) throw Error(why);
#define DL_AF_CASE(K, H)                                                                                 \
    if (a.kvMul == K && a.hs == H) {                                                                     \
        allowLds((const void *)attnDecodeF32MfmaKernel<K, H>, kAfLds);                                   \
        hipLaunchKernelGGL((attnDecodeF32MfmaKernel<K, H>), grid, dim3(kAfThreads), kAfLds, s, a);       \
        return;                                                                                          \
    }
    DL_AF_CASE(1, 128) DL_AF_CASE(2, 128) DL_AF_CASE(4, 128) DL_AF_CASE(8, 128)
    DL_AF_CASE(1, 64) DL_AF_CASE(2, 64) DL_AF_CASE(4, 64) DL_AF_CASE(8, 64)
#undef DL_AF_CASE
    throw Error("launchAttentionMfma: unsupported head size or kvMul (f32 cache)");
}

}  // namespace hipk
}  // namespace dl
