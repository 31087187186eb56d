// fthe_mul192: out[g] = x[g] y[g] mod N for N = n^2 of a Paillier-3072 key (n of 3041..3072 bits, N of 6081..6144),
// canonical little-endian rows of 192 dwords in and out, any row value accepted (rows >= N too), the result in
// [0, N).  tools/mul192_model.py is the bit-exact model of the arithmetic, DESIGN.md 22 the write-up.
//
// Eight lanes per ciphertext (lane l of the octet owns limbs [29 l, 29 l + 29) of 27 bits: 232 limbs), eight
// ciphertexts per wave, eight waves per workgroup, one persistent workgroup per CU; its waves take batches of
// eight rows from a counter in LDS.
//
//   1. rows -> LDS -> limbs: x in registers, y as the octet's multiplier column in LDS.
//   2. z = x y by operand scanning: step s multiplies the lane's 29 limbs by y[s] (one LDS broadcast) into a ring
//      of 29 64-bit columns (lane l holds columns 29 l + s .. 29 l + s + 28); the lowest column is complete for the
//      lane and moves one lane down by DPP (lane 7 takes a fresh 0), lane 0's retires as limb s of z through a
//      carry chain into the LDS word whose multiplier was just consumed.  A column sums at most 232 products
//      below 2^54: no carry is needed before a column retires.  232 more steps without products drain the ring.
//   3. Barrett on the VALU with the same routine: q = ((z >> 27*225) mu) >> 27*231 with mu = floor(2^12312 / N)
//      is floor(z / N) or one less, then r = (z - q N) mod 2^(27*228) in [0, 2N): the third
//      product retires its limbs straight into the borrow chain of z - q N.
//   4. r -> dwords (lane l: dwords [24 l, 24 l + 24); r < 2N may have bit 6144 set, which stays in its limb), one
//      conditional subtraction of N mod 2^6144 with the borrow resolved across the octet, rows stored.  Every operand row of a batch is loaded before any is stored.
//
// fthe_gprod192, below it, is the gathered 8-way product on the same routines: steps 2 and 3 per member with the
// remainder kept in LDS as the next multiplier, steps 1 and 4 once per group.  fthe_pow192, the third
// kernel, walks a whole exponent that way: x^e t by sliding windows over a table of odd powers.
// fthe_inv192_up and fthe_inv192_down are one level of a radix-8 batched inverse; fthe_horner192, the
// last, is the Horner walk over planes of rows behind the slot compress.
#include <algorithm>
#include <utility>

#include "mul192_image.hpp"

namespace mul192 {
namespace {

constexpr uint32_t kMask = (1u << kLimbBits) - 1;
constexpr int kRowStride = 2 * kLimbs + 1;     // LDS words per ciphertext: 464 limbs; odd: the rows of a wave
                                               // land in distinct banks
constexpr int kStage = kLimbs;                 // an operand row's dwords are staged at words [232, 232 + 196)
constexpr int kCtxWords = kCtxBytes / 4;
constexpr int kRLimbs = 228;                   // r < 2N < 2^(27 * 228)
enum { kFull = 0, kHigh = 1, kSub = 2 };

// f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>): the ring of columns is indexed by constants only
template <class F, int... I>
__device__ inline void static_for(F &&f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ inline void static_for(F &&f) {
    static_for(f, std::make_integer_sequence<int, N>{});
}

__device__ inline void wave_sync() {           // LDS written by one lane of the wave, read by another
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the value of the next lane of the octet; 0 in its top lane
__device__ inline uint64_t from_above(uint64_t v, bool top) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x101, 0xf, 0xf, true);          // row_shl:1
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x101, 0xf, 0xf, true);
    return top ? 0 : ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// The 464 limbs of x m (m: 232 multiplier limbs in LDS) through lane 0's carry chain into area:
//   kFull  all of them (m may be area itself: limb s lands on multiplier s after it was read);
//   kHigh  limbs 231 .. 463 only (area[0, 228) is kept);
//   kSub   area[s] = limb s of (area - x m) mod 2^(27 * 228), zero up to limb 231; no high half.
template <int MODE>
__device__ inline void product(const uint32_t (&x)[kPerLane], const uint32_t *m, uint32_t *area, bool lane0, bool top) {
    uint64_t acc[kPerLane];
#pragma unroll
    for (int i = 0; i < kPerLane; i++) acc[i] = 0;
    uint64_t carry = 0;
    uint32_t borrow = 0;
#pragma unroll 1
    for (int b = 0; b < kLanes; b++) {
        const uint32_t *mb = m + kPerLane * b;
        uint32_t *ob = area + kPerLane * b;
        static_for<kPerLane>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            const uint32_t ys = mb[t];
            static_for<kPerLane>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                acc[(t + i) % kPerLane] += (uint64_t)x[i] * ys;
            });
            carry += acc[t];
            uint32_t limb = (uint32_t)carry & kMask;
            carry >>= kLimbBits;
            if (MODE == kSub) {
                const uint32_t d = ob[t] - limb - borrow;
                borrow = d >> 31;
                limb = kPerLane * b + t < kRLimbs ? d & kMask : 0;
            }
            if (lane0 && (MODE != kHigh || kPerLane * b + t >= kShiftB)) ob[t] = limb;
            acc[t] = from_above(acc[t], top);
        });
    }
    if (MODE == kSub) return;
#pragma unroll 1
    for (int b = 0; b < kLanes; b++) {
        uint32_t *ob = area + kLimbs + kPerLane * b;
        static_for<kPerLane>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            carry += acc[t];
            if (lane0) ob[t] = (uint32_t)carry & kMask;
            carry >>= kLimbBits;
            acc[t] = from_above(acc[t], top);
        });
    }
}

// a row's dwords (lane l holds the 16-byte pieces 8 k + l) -> the staging words, zero padded for the limb reads
__device__ inline void stage(uint32_t *area, const uint4 (&v)[6], int l) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
        uint32_t *p = area + kStage + 4 * (8 * k + l);
        p[0] = v[k].x; p[1] = v[k].y; p[2] = v[k].z; p[3] = v[k].w;
    }
    if (l < 4) area[kStage + kWords + l] = 0;
}

// The lane index as a value the compiler cannot trace to the loop's invariants: the bit offsets and word indices
// derived from it are then computed where they are used, not hoisted out of the batch loop and kept (spilled)
// across the three products.
__device__ inline int opaque(int l) {
    asm volatile("" : "+v"(l));
    return l;
}

// the lane's 29 limbs of the staged row
__device__ inline void limbs_of(const uint32_t *area, int l, uint32_t (&x)[kPerLane]) {
    l = opaque(l);
#pragma unroll
    for (int i = 0; i < kPerLane; i++) {
        const uint32_t bit = (uint32_t)kLimbBits * (uint32_t)(kPerLane * l + i), w = bit >> 5;
        const uint64_t v = (uint64_t)area[kStage + w] | (uint64_t)area[kStage + w + 1] << 32;
        x[i] = (uint32_t)(v >> (bit & 31)) & kMask;
    }
}

__device__ inline void load_row(const uint32_t *base, uint64_t row, int l, uint4 (&v)[6]) {
    if (base) {
        const uint4 *p = (const uint4 *)(base + row * kWords);
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = p[8 * k + l];
    } else {                                   // the integer 1
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = make_uint4(0, 0, 0, 0);
        if (l == 0) v[0].x = 1;
    }
}

// Step 3: z as 464 limbs in area -> r = z - q N in [0, 2N) as limbs in area[0, 228), limbs 228 .. 231 zero: the
// form of a multiplier column.  xl is scratch.
__device__ inline void barrett(uint32_t (&xl)[kPerLane], uint32_t *area, const uint32_t *s_mu, const uint32_t *s_nl, int l,
                               bool lane0, bool top) {
    wave_sync();
#pragma unroll
    for (int i = 0; i < kPerLane; i++) xl[i] = area[kShiftA + kPerLane * l + i];
    wave_sync();
    product<kHigh>(xl, s_mu, area, lane0, top);                     // (z >> 27*225) mu
    wave_sync();
#pragma unroll
    for (int i = 0; i < kPerLane; i++) xl[i] = area[kShiftB + kPerLane * l + i];
    wave_sync();
    product<kSub>(xl, s_nl, area, lane0, top);                      // r = z - q N
    wave_sync();
}

// Step 4: r in [0, 2N) as limbs in area[0, 228) -> the lane's 24 dwords of r mod N (lane l: dwords [24 l, 24 l + 24))
__device__ inline void canonical_dwords(const uint32_t *area, const uint32_t *s_nd, int l, bool lane0, uint32_t (&r)[24]) {
    const int lo = opaque(l);
    const uint32_t *nd = s_nd + 24 * lo;
#pragma unroll
    for (int k = 0; k < 24; k++) {
        const uint32_t bit = 32u * (uint32_t)(24 * lo + k), j = bit / kLimbBits;
        const uint64_t v = (uint64_t)area[j] | (uint64_t)area[j + 1] << 27 | (uint64_t)area[j + 2] << 54;
        r[k] = (uint32_t)(v >> (bit - kLimbBits * j));
    }
    // r - N: the lane's own borrow g, and whether a borrow from below passes through (the difference is 0)
    uint32_t g = 0, any = 0;
#pragma unroll
    for (int k = 0; k < 24; k++) {
        const uint64_t d = (uint64_t)r[k] - nd[k] - g;
        g = (uint32_t)(d >> 63);
        any |= (uint32_t)d;
    }
    const uint32_t pass = any == 0 ? 1u : 0u;
    uint32_t bin = 0, bout = g;
#pragma unroll
    for (int it = 0; it < kLanes - 1; it++) {
        const uint32_t up = __shfl_up(bout, 1, kLanes);
        bin = lane0 ? 0u : up;
        bout = g | (bin & pass);
    }
    // r < N: the octet's last borrow, unless r has bits above the row (r < 2N may reach 2^6144: limb 227, bit 15)
    const bool keep = __shfl(bout, kLanes - 1, kLanes) != 0 && (area[kRLimbs - 1] >> (32 * kWords % kLimbBits)) == 0;
#pragma unroll
    for (int k = 0; k < 24; k++) {
        const uint64_t d = (uint64_t)r[k] - nd[k] - bin;
        bin = (uint32_t)(d >> 63);
        r[k] = keep ? r[k] : (uint32_t)d;
    }
}

__global__ __launch_bounds__(64 * kWaves) void fthe_mul192_kernel(const uint32_t *x, const uint32_t *y, uint32_t *out,
                                                                  const uint32_t *kctx, uint32_t count, uint32_t nwg) {
    __shared__ uint32_t s_ctx[kCtxWords];                       // mu limbs, N limbs, N dwords
    __shared__ uint32_t s_rows[kPerWg * kRowStride];
    __shared__ uint32_t s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 7, oct = lane >> 3;
    for (int i = tid; i < kCtxWords; i += 64 * kWaves) s_ctx[i] = kctx[i];
    if (tid == 0) s_next = 0;
    __syncthreads();
    const uint32_t *s_mu = s_ctx + kMuOff / 4, *s_nl = s_ctx + kNlOff / 4, *s_nd = s_ctx + kNdOff / 4;
    uint32_t *area = s_rows + (wave * kRowsPerWave + oct) * kRowStride;
    const bool lane0 = l == 0, top = l == kLanes - 1;
    const uint32_t nbatch = (count + kRowsPerWave - 1) / kRowsPerWave;
    for (;;) {
        // workgroup wg owns batches wg, wg + nwg, ...; its waves take them in turn
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(&s_next, 1u);
        t = __builtin_amdgcn_readfirstlane(t);
        const uint64_t batch = blockIdx.x + (uint64_t)t * nwg;
        if (batch >= nbatch) break;
        uint64_t row = batch * kRowsPerWave + oct;
        const bool live = row < count;
        if (!live) row = count - 1;            // an idle octet repeats the last row and stores nothing
        // one operand at a time through the staging words (few registers live at once); both are loaded before
        // the batch stores anything
        uint4 v[6];
        uint32_t xl[kPerLane];
        load_row(y, row, l, v);
        stage(area, v, l);
        load_row(x, row, l, v);
        wave_sync();
        limbs_of(area, l, xl);                 // y's limbs: the multiplier column (not the staging words)
#pragma unroll
        for (int i = 0; i < kPerLane; i++) area[kPerLane * l + i] = xl[i];
        wave_sync();
        stage(area, v, l);
        wave_sync();
        limbs_of(area, l, xl);
        wave_sync();
        product<kFull>(xl, area, area, lane0, top);                     // z
        barrett(xl, area, s_mu, s_nl, l, lane0, top);
        uint32_t r[24];
        canonical_dwords(area, s_nd, l, lane0, r);
        if (live) {
            uint4 *p = (uint4 *)(out + row * kWords + 24 * l);
#pragma unroll
            for (int k = 0; k < 6; k++) p[k] = make_uint4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
        }
        wave_sync();
    }
}

// fthe_gprod192: out[g] = prod_{j < 8} src[gidx[j G + g]] mod N (an index below 0: the integer 1), the gathered
// product behind the segmented products, the histogram and the segmented scan.  The geometry above;
// an octet owns group g and walks its members with the running product resident in LDS:
//
//   member 0 -> staging words -> limbs -> the octet's multiplier column area[0, 232);
//   step j = 1 ..: member j -> staging words -> limbs x in registers, z = x r (kFull, the multiplier column being r),
//   then step 3 above, which leaves r in [0, 2N) where the next step's multiplier column is read: no dwords, no
//   conditional subtraction, no store and no reload between members.  r < 2N <= 2^6145 makes z < 2^12289, one bit
//   above a product of two rows; the cut points hold for it (tools/mul192_model.py chain()).
//   After the last step only: step 4 and the store.
//
// The product routine is wave-wide, so a wave runs max(2, members of its longest group) - 1 steps; an octet without
// a member j multiplies by 1 there.  At least one step: a lone member >= N comes out reduced, no member gives 1.
// Lane j of an octet holds the group's index j (K = 8 = the lanes of an octet) until the steps are counted; each
// step then reads its index again, which keeps two registers free across the products.  Every member of a wave's
// batch is read before the batch stores; across batches dst must not overlap src.
constexpr int kGather = kLanes;

__global__ __launch_bounds__(64 * kWaves) void fthe_gprod192_kernel(const uint32_t *src, const int64_t *gidx, uint32_t *dst,
                                                                    const uint32_t *kctx, uint64_t count, uint32_t nwg) {
    __shared__ uint32_t s_ctx[kCtxWords];                       // mu limbs, N limbs, N dwords
    __shared__ uint32_t s_rows[kPerWg * kRowStride];
    __shared__ uint32_t s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 7, oct = lane >> 3;
    for (int i = tid; i < kCtxWords; i += 64 * kWaves) s_ctx[i] = kctx[i];
    if (tid == 0) s_next = 0;
    __syncthreads();
    const uint32_t *s_mu = s_ctx + kMuOff / 4, *s_nl = s_ctx + kNlOff / 4, *s_nd = s_ctx + kNdOff / 4;
    uint32_t *area = s_rows + (wave * kRowsPerWave + oct) * kRowStride;
    const bool lane0 = l == 0, top = l == kLanes - 1;
    const uint64_t nbatch = (count + kRowsPerWave - 1) / kRowsPerWave;
    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(&s_next, 1u);
        t = __builtin_amdgcn_readfirstlane(t);
        const uint64_t batch = blockIdx.x + (uint64_t)t * nwg;
        if (batch >= nbatch) break;
        const uint64_t g = batch * kRowsPerWave + oct;
        const bool live = g < count;           // an idle octet has no member: it multiplies 1 by 1 and stores nothing
        // the wave's step count: one more than the highest member position that any of its octets fills
        const int64_t mine = live ? gidx[(uint64_t)l * count + g] : -1;
        const uint64_t has = __ballot(mine >= 0);
        uint32_t pos = (uint32_t)has | (uint32_t)(has >> 32);
        pos |= pos >> 16;
        pos = (pos | pos >> 8) & 0xffu;
        const int members = __builtin_amdgcn_readfirstlane(32 - __builtin_clz(pos | 1u));
        uint4 v[6];
        uint32_t xl[kPerLane];
        int64_t at = __shfl(mine, 0, kLanes);
        load_row(at >= 0 ? src : nullptr, (uint64_t)at, l, v);
        stage(area, v, l);
        wave_sync();
        limbs_of(area, l, xl);
#pragma unroll
        for (int i = 0; i < kPerLane; i++) area[kPerLane * l + i] = xl[i];
        wave_sync();
#pragma unroll 1
        for (int j = 1; j < (members < 2 ? 2 : members); j++) {
            at = live ? gidx[(uint64_t)j * count + g] : -1;
            load_row(at >= 0 ? src : nullptr, (uint64_t)at, l, v);
            stage(area, v, l);                 // over the spent high limbs of the step before
            wave_sync();
            limbs_of(area, l, xl);
            wave_sync();
            product<kFull>(xl, area, area, lane0, top);                 // z = x r
            barrett(xl, area, s_mu, s_nl, l, lane0, top);
        }
        uint32_t r[24];
        canonical_dwords(area, s_nd, l, lane0, r);
        if (live) {
            uint4 *p = (uint4 *)(dst + g * kWords + 24 * l);
#pragma unroll
            for (int k = 0; k < 6; k++) p[k] = make_uint4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
        }
        wave_sync();
    }
}

// fthe_pow192: out[g] = x[g]^e t[g] mod N for one exponent e >= 2 shared by the batch (t null: 1), the power behind
// the public-key encrypt r^n (1 + m n) and the uniform scalar mul.  The geometry above; an octet owns
// one row for the whole walk, with the running value resident in LDS as the multiplier column, as in fthe_gprod192:
//
//   base: a row of xw <= 192 words, zero-extended -> staging words -> limbs x in registers; one product by the
//   column 1 and step 3 leave x as a lazy remainder in [0, 2N) in area[0, 228).
//   table: odd powers x^1, x^3, ..., entry j = x^(2 j - 1), as lazy limb rows in global memory, the lane's 29 limbs
//   padded to 32 words (eight 16-byte pieces), one table per slot (workgroup, wave, octet).  A lane reads back only
//   what it wrote itself.  x^2 is formed once and parked in the last entry's place; entry k + 1 = x^2 * entry k with
//   entry k still lying in area as the multiplier column (k = 1: the column is x^2, the registers hold entry 1), the
//   last product overwriting x^2's place.
//   walk: the host's byte string (pow_schedule), read with scalar loads: byte 0 names the entry that becomes the
//   column; then 0 = square, the registers taking the column itself (xl[i] = area[29 l + i]: nothing is re-limbed),
//   j = multiply, the registers taking entry j from global memory; each is product<kFull>(xl, area, area) and step 3.
//   Nothing is converted, subtracted or stored between products.  Both factors are lazy now: z < 2^12290, for which
//   the cut points hold (tools/mul192_model.py power()).
//   tail: t's row through the staging words as a gathered member, one more product; then step 4 and the store.
//
// A row is read and written by its octet alone, the base before anything else and t after the walk: out may be
// exactly t, or exactly x when xw = 192.  An idle octet of the last batch repeats the last row and stores nothing.
__device__ inline void load_base(const uint32_t *x, int xw, bool vec, uint64_t row, int l, uint4 (&v)[6]) {
    const uint32_t *p = x + row * (uint64_t)xw;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int w0 = 4 * (8 * k + l);
        if (vec) {
            v[k] = w0 < xw ? *(const uint4 *)(p + w0) : make_uint4(0, 0, 0, 0);
        } else {
            v[k].x = w0 < xw ? p[w0] : 0;
            v[k].y = w0 + 1 < xw ? p[w0 + 1] : 0;
            v[k].z = w0 + 2 < xw ? p[w0 + 2] : 0;
            v[k].w = w0 + 3 < xw ? p[w0 + 3] : 0;
        }
    }
}

// the lane's limbs of the multiplier column (a lazy remainder) -> registers
__device__ inline void column_of(const uint32_t *area, int l, uint32_t (&xl)[kPerLane]) {
    const uint32_t *a = area + kPerLane * opaque(l);
#pragma unroll
    for (int i = 0; i < kPerLane; i++) xl[i] = a[i];
}

// the lane's 128 bytes of table entry j (from 0) of its octet's table
__device__ inline uint4 *entry_at(uint32_t *table, uint32_t slot0, uint32_t stride, uint32_t j, int lane) {
    const int ln = opaque(lane);
    return (uint4 *)(table + ((uint64_t)(slot0 + (ln >> 3)) * stride + j) * kEntryWords + 32 * (ln & 7));
}
__device__ inline void entry_store(uint4 *e, const uint32_t *area, int l) {
    const uint32_t *a = area + kPerLane * opaque(l);
#pragma unroll
    for (int k = 0; k < 7; k++) e[k] = make_uint4(a[4 * k], a[4 * k + 1], a[4 * k + 2], a[4 * k + 3]);
    e[7] = make_uint4(a[28], 0, 0, 0);
}
__device__ inline void entry_load(const uint4 *e, uint32_t (&xl)[kPerLane]) {
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const uint4 q = e[k];
        xl[4 * k] = q.x; xl[4 * k + 1] = q.y; xl[4 * k + 2] = q.z; xl[4 * k + 3] = q.w;
    }
    xl[28] = e[7].x;
}

__global__ __launch_bounds__(64 * kWaves) void fthe_pow192_kernel(const uint32_t *x, int xw, int vec, const uint32_t *t,
                                                                  uint32_t *out, const uint32_t *kctx,
                                                                  const uint32_t *__restrict__ sched, uint32_t slen,
                                                                  uint32_t *table, uint32_t stride, uint32_t entries,
                                                                  uint64_t count, uint32_t nwg) {
    __shared__ uint32_t s_ctx[kCtxWords];                       // mu limbs, N limbs, N dwords
    __shared__ uint32_t s_rows[kPerWg * kRowStride];
    __shared__ uint32_t s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 7, oct = lane >> 3;
    for (int i = tid; i < kCtxWords; i += 64 * kWaves) s_ctx[i] = kctx[i];
    if (tid == 0) s_next = 0;
    __syncthreads();
    const uint32_t *s_mu = s_ctx + kMuOff / 4, *s_nl = s_ctx + kNlOff / 4, *s_nd = s_ctx + kNdOff / 4;
    uint32_t *area = s_rows + (wave * kRowsPerWave + oct) * kRowStride;
    const bool lane0 = l == 0, top = l == kLanes - 1;
    const uint32_t slot0 = __builtin_amdgcn_readfirstlane((blockIdx.x * kWaves + wave) * kRowsPerWave);
    const uint64_t nbatch = (count + kRowsPerWave - 1) / kRowsPerWave;
    for (;;) {
        uint32_t tk = 0;
        if (lane == 0) tk = atomicAdd(&s_next, 1u);
        tk = __builtin_amdgcn_readfirstlane(tk);
        const uint64_t batch = blockIdx.x + (uint64_t)tk * nwg;
        if (batch >= nbatch) break;
        // the octet's row, recomputed where it is used rather than kept across the products
        auto row_of = [&](bool &live) {
            uint64_t row = batch * kRowsPerWave + (uint32_t)(opaque(lane) >> 3);
            live = row < count;
            return live ? row : count - 1;
        };
        uint32_t xl[kPerLane];
        {
            bool live;
            uint4 v[6];
            load_base(x, xw, vec != 0, row_of(live), l, v);
            stage(area, v, l);
        }
        wave_sync();
        // One product site for the whole walk; every condition below is uniform.  Steps [0, nbuild): the base by 1
        // (-> entry 1), then x^2 (parked in the last entry's place) and x^2 times the entry before (-> entries 2 ..);
        // steps [nbuild, nbuild + slen - 1): the schedule's bytes 1 ..; a last step for t.
        const uint32_t nbuild = entries > 1 ? entries + 1 : 1, nwalk = nbuild + slen - 1, total = nwalk + (t ? 1 : 0);
#pragma unroll 1
        for (uint32_t s = 0; s < total; s++) {
            if (s == 0 || s >= nwalk) {
                if (s) {
                    bool live;
                    uint4 v[6];
                    load_row(t, row_of(live), l, v);
                    stage(area, v, l);             // over the spent high limbs of the step before
                    wave_sync();
                }
                limbs_of(area, l, xl);
                wave_sync();
                if (s == 0) {
#pragma unroll
                    for (int i = 0; i < kPerLane; i++) area[kPerLane * l + i] = (lane0 && i == 0) ? 1u : 0u;
                }
            } else {
                uint32_t j = 0;                    // 0: square, else times entry j
                if (s >= nbuild) {
                    const uint32_t i = s - nbuild + 1;
                    j = (sched[i >> 2] >> (8 * (i & 3))) & 0xffu;
                } else if (s > 1) {
                    j = s == 2 ? 1 : entries;
                }
                j = __builtin_amdgcn_readfirstlane(j);
                if (j == 0) column_of(area, l, xl);
                else entry_load(entry_at(table, slot0, stride, j - 1, lane), xl);
            }
            wave_sync();
            product<kFull>(xl, area, area, lane0, top);
            barrett(xl, area, s_mu, s_nl, l, lane0, top);
            if (s < nbuild) {
                entry_store(entry_at(table, slot0, stride, s == 0 ? 0 : s == 1 ? entries - 1 : s - 1, lane), area, l);
                if (s + 1 == nbuild) {             // the table is whole: the schedule's first byte names the seed
                    entry_load(entry_at(table, slot0, stride, (sched[0] & 0xffu) - 1, lane), xl);
                    wave_sync();
#pragma unroll
                    for (int i = 0; i < kPerLane; i++) area[kPerLane * l + i] = xl[i];
                    wave_sync();
                }
            }
        }
        uint32_t r[24];
        canonical_dwords(area, s_nd, l, lane0, r);
        bool live;
        const uint64_t row = row_of(live);
        if (live) {
            uint4 *p = (uint4 *)(out + row * kWords + 24 * l);
#pragma unroll
            for (int k = 0; k < 6; k++) p[k] = make_uint4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
        }
        wave_sync();
    }
}

// fthe_inv192_up / fthe_inv192_down: one level of the radix-8 tree of Montgomery's trick, the batched inverse behind
// fthe_invert and fthe_sub_inv (tools/mul192_model.py inverse()).  The geometry above; an octet owns
// group g, the rows [8 g, 8 g + 8) of a level of `count` rows x (a row past the level's end: the integer 1), and walks
// it with the running value resident in LDS as the multiplier column.  Level rows are canonical rows of 192 words;
// what a group keeps for itself are lazy limb rows in fthe_pow192's entry format, which a lane reads back as it wrote
// them.  Every product has factors below 2^6145: fthe_pow192's case, the same cut points.
//
//   up:    p_0 = x_0 -> the column and prefix entry 0; steps j = 1 .. 7: p_j = p_(j-1) x_j, x_j through the staging
//          words, p_j -> prefix entry j (j < 7); the total p_7 -> step 4 -> row g of the level above.
//   down:  R_7 = row g of the level above, inverted: the inverse of p_7 -> the column.  For j = 7 .. 1:
//            A  the column R_j is parked in the octet's slot entry (the product consumes it; neither 29 more registers
//               nor a second LDS area are to be had), I_j = R_j p_(j-1), the prefix entry in the registers;
//            T  with a: I_j a_j, a_j through the staging words;
//            B  x_j is staged over the spent high limbs, then step 4 and the store of row 8 g + j of out, then the
//               column is R_j again from the slot and R_(j-1) = R_j x_j.
//          I_0 = R_0 (T with a), step 4, row 8 g.  Row 8 g + j of x and of a is read before row 8 g + j of out is
//          stored, and row 8 g of x is not read at all (p_0 is its copy): out may be exactly x or a.  One product site;
//          every condition on the step is uniform.
// An idle octet of the last batch repeats the last group and stores nothing.
__device__ inline uint4 *prefix_at(uint32_t *pre, uint64_t g, uint32_t j, int l) {
    return (uint4 *)(pre + (g * (kGather - 1) + j) * kEntryWords + 32 * opaque(l));
}
__device__ inline void column_from(uint32_t *area, int l, const uint32_t (&xl)[kPerLane]) {
    uint32_t *a = area + kPerLane * opaque(l);
#pragma unroll
    for (int i = 0; i < kPerLane; i++) a[i] = xl[i];
}
__device__ inline void store_row(uint32_t *out, uint64_t row, int l, const uint32_t (&r)[24]) {
    uint4 *p = (uint4 *)(out + row * kWords + 24 * l);
#pragma unroll
    for (int k = 0; k < 6; k++) p[k] = make_uint4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
}

__global__ __launch_bounds__(64 * kWaves) void fthe_inv192_up_kernel(const uint32_t *x, uint32_t *pre, uint32_t *dst,
                                                                     const uint32_t *kctx, uint64_t count, uint32_t nwg) {
    __shared__ uint32_t s_ctx[kCtxWords];                       // mu limbs, N limbs, N dwords
    __shared__ uint32_t s_rows[kPerWg * kRowStride];
    __shared__ uint32_t s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 7, oct = lane >> 3;
    for (int i = tid; i < kCtxWords; i += 64 * kWaves) s_ctx[i] = kctx[i];
    if (tid == 0) s_next = 0;
    __syncthreads();
    const uint32_t *s_mu = s_ctx + kMuOff / 4, *s_nl = s_ctx + kNlOff / 4, *s_nd = s_ctx + kNdOff / 4;
    uint32_t *area = s_rows + (wave * kRowsPerWave + oct) * kRowStride;
    const bool lane0 = l == 0, top = l == kLanes - 1;
    const uint64_t groups = (count + kGather - 1) / kGather, nbatch = (groups + kRowsPerWave - 1) / kRowsPerWave;
    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(&s_next, 1u);
        t = __builtin_amdgcn_readfirstlane(t);
        const uint64_t batch = blockIdx.x + (uint64_t)t * nwg;
        if (batch >= nbatch) break;
        uint64_t g = batch * kRowsPerWave + oct;
        const bool live = g < groups;
        if (!live) g = groups - 1;
        uint4 v[6];
        uint32_t xl[kPerLane];
        load_row(x, g * kGather, l, v);
        stage(area, v, l);
        wave_sync();
        limbs_of(area, l, xl);
        column_from(area, l, xl);
        wave_sync();
        if (live) entry_store(prefix_at(pre, g, 0, l), area, l);
#pragma unroll 1
        for (int j = 1; j < kGather; j++) {
            const uint64_t row = g * kGather + j;
            load_row(row < count ? x : nullptr, row, l, v);
            stage(area, v, l);                 // over the spent high limbs of the step before
            wave_sync();
            limbs_of(area, l, xl);
            wave_sync();
            product<kFull>(xl, area, area, lane0, top);                 // z = x_j p_(j-1)
            barrett(xl, area, s_mu, s_nl, l, lane0, top);
            if (live && j < kGather - 1) entry_store(prefix_at(pre, g, j, l), area, l);
        }
        uint32_t r[24];
        canonical_dwords(area, s_nd, l, lane0, r);
        if (live) store_row(dst, g, l, r);
        wave_sync();
    }
}

__global__ __launch_bounds__(64 * kWaves) void fthe_inv192_down_kernel(const uint32_t *x, const uint32_t *a,
                                                                       const uint32_t *inv, uint32_t *pre, uint32_t *park,
                                                                       uint32_t *out, const uint32_t *kctx, uint64_t count,
                                                                       uint32_t nwg) {
    __shared__ uint32_t s_ctx[kCtxWords];                       // mu limbs, N limbs, N dwords
    __shared__ uint32_t s_rows[kPerWg * kRowStride];
    __shared__ uint32_t s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 7, oct = lane >> 3;
    for (int i = tid; i < kCtxWords; i += 64 * kWaves) s_ctx[i] = kctx[i];
    if (tid == 0) s_next = 0;
    __syncthreads();
    const uint32_t *s_mu = s_ctx + kMuOff / 4, *s_nl = s_ctx + kNlOff / 4, *s_nd = s_ctx + kNdOff / 4;
    uint32_t *area = s_rows + (wave * kRowsPerWave + oct) * kRowStride;
    const bool lane0 = l == 0, top = l == kLanes - 1;
    const uint32_t slot0 = __builtin_amdgcn_readfirstlane((blockIdx.x * kWaves + wave) * kRowsPerWave);
    const uint64_t groups = (count + kGather - 1) / kGather, nbatch = (groups + kRowsPerWave - 1) / kRowsPerWave;
    const uint32_t per = a ? 3 : 2, total = (kGather - 1) * per + (a ? 1 : 0);
    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(&s_next, 1u);
        t = __builtin_amdgcn_readfirstlane(t);
        const uint64_t batch = blockIdx.x + (uint64_t)t * nwg;
        if (batch >= nbatch) break;
        // the octet's group, recomputed where it is used rather than kept across the products
        auto group_of = [&](bool &live) {
            const uint64_t g = batch * kRowsPerWave + (uint32_t)(opaque(lane) >> 3);
            live = g < groups;
            return live ? g : groups - 1;
        };
        uint32_t xl[kPerLane];
        {
            bool live;
            uint4 v[6];
            load_row(inv, group_of(live), l, v);
            stage(area, v, l);
            wave_sync();
            limbs_of(area, l, xl);
            column_from(area, l, xl);                                   // R_7
        }
#pragma unroll 1
        for (uint32_t s = 0; s < total; s++) {
            const uint32_t j = (kGather - 1) - s / per, ph = s - (kGather - 1 - j) * per;
            bool live;
            const uint64_t g = group_of(live), row = g * kGather + j;
            wave_sync();
            if (j && ph == 0) {                                         // A
                uint4 *slot = entry_at(park, slot0, 1, 0, lane);
                entry_store(slot, area, l);
                entry_load(prefix_at(pre, g, j - 1, l), xl);
            } else {
                uint4 v[6];
                const bool tail = !j || ph + 1 < per;                   // T, else B
                load_row(row < count ? (tail ? a : x) : nullptr, row, l, v);
                stage(area, v, l);                 // over the spent high limbs of the step before
                if (!tail) {
                    uint32_t r[24];
                    canonical_dwords(area, s_nd, l, lane0, r);
                    if (live && row < count) store_row(out, row, l, r);
                    entry_load(entry_at(park, slot0, 1, 0, lane), xl);
                    wave_sync();
                    column_from(area, l, xl);                           // R_j again
                }
                wave_sync();
                limbs_of(area, l, xl);
            }
            wave_sync();
            product<kFull>(xl, area, area, lane0, top);
            barrett(xl, area, s_mu, s_nl, l, lane0, top);
        }
        uint32_t r[24];
        canonical_dwords(area, s_nd, l, lane0, r);
        bool live;
        const uint64_t g = group_of(live);
        if (live) store_row(out, g * kGather, l, r);
        wave_sync();
    }
}

// fthe_horner192: out[i] = prod_{j < planes} x[j stride + i]^(2^(j sq)) mod N, the Horner walk behind the compress of
// pair-packed into slot-packed ciphertexts (tools/mul192_model.py horner()).  planes >= 2 and sq >= 1
// are the launch's: every wave runs the same 1 + (planes - 1)(sq + 1) products.  The geometry above; an octet owns
// output row i for the whole walk, with the running value resident in LDS as the multiplier column:
//
//   seed: the top plane's row -> staging words -> limbs x in registers; one product by the column 1 and step 3 leave it
//   as a lazy remainder in [0, 2N) in area[0, 228): fthe_pow192's base step.
//   per plane below the top: sq squarings, the registers taking the column itself (column_of: nothing is re-limbed),
//   then one product by that plane's row, loaded at that step and staged over the spent high limbs as fthe_pow192's
//   tail stages t.  (Loading it one squaring ahead holds 24 registers across a product: 256 VGPRs and 8 spilled
//   against 240 and none, for one row's latency per sq + 1 products.)
//   Nothing is converted, subtracted or stored between products; both factors are below 2^6145, a staged row below
//   2^6144: fthe_pow192's case, the same cut points.  After the last product only: step 4 and the store.
//
// One product site; every condition on the step is uniform.  A row of out is written by its octet alone, after every
// row of x that the octet reads: out must not overlap x all the same, since other octets read other planes of the
// same rows later.  An idle octet of the last batch repeats the last row and stores nothing.
__global__ __launch_bounds__(64 * kWaves) void fthe_horner192_kernel(const uint32_t *x, uint64_t stride, uint32_t planes,
                                                                     uint32_t sq, uint32_t *out, const uint32_t *kctx,
                                                                     uint64_t count, uint32_t nwg) {
    __shared__ uint32_t s_ctx[kCtxWords];                       // mu limbs, N limbs, N dwords
    __shared__ uint32_t s_rows[kPerWg * kRowStride];
    __shared__ uint32_t s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 7, oct = lane >> 3;
    for (int i = tid; i < kCtxWords; i += 64 * kWaves) s_ctx[i] = kctx[i];
    if (tid == 0) s_next = 0;
    __syncthreads();
    const uint32_t *s_mu = s_ctx + kMuOff / 4, *s_nl = s_ctx + kNlOff / 4, *s_nd = s_ctx + kNdOff / 4;
    uint32_t *area = s_rows + (wave * kRowsPerWave + oct) * kRowStride;
    const bool lane0 = l == 0, top = l == kLanes - 1;
    const uint64_t nbatch = (count + kRowsPerWave - 1) / kRowsPerWave;
    const uint32_t total = 1 + (planes - 1) * (sq + 1);
    for (;;) {
        uint32_t tk = 0;
        if (lane == 0) tk = atomicAdd(&s_next, 1u);
        tk = __builtin_amdgcn_readfirstlane(tk);
        const uint64_t batch = blockIdx.x + (uint64_t)tk * nwg;
        if (batch >= nbatch) break;
        // the octet's row, recomputed where it is used rather than kept across the products
        auto row_of = [&](bool &live) {
            uint64_t row = batch * kRowsPerWave + (uint32_t)(opaque(lane) >> 3);
            live = row < count;
            return live ? row : count - 1;
        };
        uint32_t xl[kPerLane];
        bool live;
        {
            uint4 v[6];
            load_row(x + (uint64_t)(planes - 1) * stride * kWords, row_of(live), l, v);
            stage(area, v, l);
        }
        wave_sync();
        // u: squarings done since the last row; j: the plane whose row is multiplied next
        uint32_t u = 0, j = planes - 2;
#pragma unroll 1
        for (uint32_t s = 0; s < total; s++) {
            if (s && u < sq) {
                u++;
                column_of(area, l, xl);
            } else {
                if (s) {
                    uint4 v[6];
                    load_row(x + (uint64_t)j * stride * kWords, row_of(live), l, v);
                    stage(area, v, l);             // over the spent high limbs of the step before
                    wave_sync();
                    u = 0;
                    j--;
                }
                limbs_of(area, l, xl);
                wave_sync();
                if (s == 0) {
#pragma unroll
                    for (int i = 0; i < kPerLane; i++) area[kPerLane * l + i] = (lane0 && i == 0) ? 1u : 0u;
                }
            }
            wave_sync();
            product<kFull>(xl, area, area, lane0, top);
            barrett(xl, area, s_mu, s_nl, l, lane0, top);
        }
        uint32_t r[24];
        canonical_dwords(area, s_nd, l, lane0, r);
        const uint64_t row = row_of(live);
        if (live) store_row(out, row, l, r);
        wave_sync();
    }
}

}  // namespace

int launch_horner(hipStream_t st, const uint32_t *x, size_t stride, int planes, int sq, uint32_t *out, const void *kctx,
                  size_t count, int n_cu) {
    if (count == 0) return hipSuccess;
    if (planes < 2 || sq < 1 || stride < count) return hipErrorInvalidValue;
    const uint64_t products = horner_products(planes, sq);
    const size_t per = std::min<size_t>((size_t)pow_blocks(count, n_cu) * kPerWg *
                                            (size_t)std::max<uint64_t>(1, kPowBudget / products),
                                        (size_t)1 << 22);
    for (size_t off = 0; off < count; off += per) {
        const size_t cnt = std::min(per, count - off);
        const unsigned blocks = pow_blocks(cnt, n_cu);
        hipLaunchKernelGGL(fthe_horner192_kernel, dim3(blocks), dim3(64 * kWaves), 0, st, x + off * kWords,
                           (uint64_t)stride, (uint32_t)planes, (uint32_t)sq, out + off * kWords, (const uint32_t *)kctx,
                           (uint64_t)cnt, blocks);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

int launch_inv_up(hipStream_t st, const uint32_t *x, uint32_t *pre, uint32_t *dst, const void *kctx, size_t count,
                  int n_cu) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = inv_blocks(count, n_cu);
    hipLaunchKernelGGL(fthe_inv192_up_kernel, dim3(blocks), dim3(64 * kWaves), 0, st, x, pre, dst, (const uint32_t *)kctx,
                       (uint64_t)count, blocks);
    return hipGetLastError();
}

int launch_inv_down(hipStream_t st, const uint32_t *x, const uint32_t *a, const uint32_t *inv, uint32_t *pre,
                    uint32_t *park, uint32_t *out, const void *kctx, size_t count, int n_cu) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = inv_blocks(count, n_cu);
    hipLaunchKernelGGL(fthe_inv192_down_kernel, dim3(blocks), dim3(64 * kWaves), 0, st, x, a, inv, pre, park, out,
                       (const uint32_t *)kctx, (uint64_t)count, blocks);
    return hipGetLastError();
}

int launch_pow(hipStream_t st, const uint32_t *x, int xw, const uint32_t *t, uint32_t *out, const void *kctx,
               const uint32_t *sched, uint32_t slen, unsigned entries, uint64_t products, uint32_t *table, int w,
               size_t count, int n_cu) {
    if (count == 0) return hipSuccess;
    if (xw <= 0 || xw > kWords || w < 1 || w > kPowMaxWindow || !slen || entries < 1 || entries > (1u << (w - 1)))
        return hipErrorInvalidValue;
    const int vec = xw % 4 == 0 && (uintptr_t)x % 16 == 0;
    const unsigned blocks = pow_blocks(count, n_cu);
    const size_t per = std::min<size_t>((size_t)blocks * kPerWg * (size_t)std::max<uint64_t>(1, kPowBudget / products),
                                        (size_t)1 << 22);
    for (size_t off = 0; off < count; off += per) {
        const size_t cnt = std::min(per, count - off);
        hipLaunchKernelGGL(fthe_pow192_kernel, dim3(pow_blocks(cnt, n_cu)), dim3(64 * kWaves), 0, st,
                           x + off * (size_t)xw, xw, vec, t ? t + off * kWords : nullptr, out + off * kWords,
                           (const uint32_t *)kctx, sched, slen, table, 1u << (w - 1), entries, (uint64_t)cnt,
                           pow_blocks(cnt, n_cu));
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

int launch_gather(hipStream_t st, const uint32_t *src, const int64_t *gidx, uint32_t *dst, const void *kctx, size_t count,
                  int n_cu) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>((count + kPerWg - 1) / kPerWg, (size_t)std::max(n_cu, 1));
    hipLaunchKernelGGL(fthe_gprod192_kernel, dim3(blocks), dim3(64 * kWaves), 0, st, src, gidx, dst, (const uint32_t *)kctx,
                       (uint64_t)count, blocks);
    return hipGetLastError();
}

int launch(hipStream_t st, const uint32_t *x, const uint32_t *y, uint32_t *out, const void *kctx, size_t count, int n_cu) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>((count + kPerWg - 1) / kPerWg, (size_t)std::max(n_cu, 1));
    hipLaunchKernelGGL(fthe_mul192_kernel, dim3(blocks), dim3(64 * kWaves), 0, st, x, y, out, (const uint32_t *)kctx,
                       (uint32_t)count, blocks);
    return hipGetLastError();
}

}  // namespace mul192
