/* vox_kv8.h -- the one-byte decoder KV ring element (opt-in, VOX_HIP_KV_FP8): OCP FP8 E4M3
 * ("e4m3fn", the gfx950 native format): 1 sign, 4 exponent (bias 7), 3 mantissa bits; no
 * infinities, S.1111.111 is NaN, largest finite value 448 (S.1111.110); subnormals m * 2^-9
 * below 2^-6.
 *
 * The host statement of the rule the kernels' ring stores follow (vox_hip_dev.h, kv8_t)
 * byte for byte, for every f32 input:
 *   encode: clamp to +-448 (so +-Inf and everything at or above the overflow midpoint 464 give
 *           +-448: the ring saturates, it never stores a NaN for a finite or infinite input),
 *           then round to the nearest E4M3 value, ties to the even mantissa, subnormals kept,
 *           the sign of zero kept; NaN -> 0x7f with the input's sign bit.
 *   decode: exact (every E4M3 value is an f32).
 * There is no scale: values are stored as they are.  A per-layer power-of-two scale would
 * need a real checkpoint's K/V statistics to calibrate against and is out of scope.
 * Plain C, header only, no dependencies beyond <stdint.h> / <string.h> / <math.h>. */
#ifndef VOX_KV8_H
#define VOX_KV8_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#define VOX_KV8_MAX 448.0f

static inline uint8_t vox_kv8_encode_(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80);
    if (x != x) return (uint8_t)(sign | 0x7f);
    float a = fabsf(x);
    if (a >= VOX_KV8_MAX) return (uint8_t)(sign | 0x7e);
    if (a < 0.015625f) {
        /* subnormal range (and the step up to the first normal, code 8 = 2^-6): multiples of
         * 2^-9; a * 512 is exact, nearbyintf rounds ties to even in the default mode */
        return (uint8_t)(sign | (uint8_t)nearbyintf(a * 512.0f));
    }
    memcpy(&u, &a, 4);
    /* normal: keep 3 mantissa bits of the 23, nearest, ties to even; a mantissa carry moves
     * into the exponent by the addition (a < 448 cannot pass code 0x7e: 447.99.. -> 448) */
    const uint32_t lsb = (u >> 20) & 1;
    u += 0x7ffffu + lsb;
    const int e = (int)(u >> 23) - 127 + 7; /* 1..15 */
    return (uint8_t)(sign | (uint8_t)(e << 3) | (uint8_t)((u >> 20) & 7));
}

static inline float vox_kv8_decode_(uint8_t c) {
    const int e = (c >> 3) & 15, m = c & 7;
    float v;
    if (e == 15 && m == 7) {
        uint32_t u = 0x7fc00000u | ((uint32_t)(c & 0x80) << 24);
        memcpy(&v, &u, 4);
        return v;
    }
    v = e ? ldexpf((float)(8 + m), e - 10) : ldexpf((float)m, -9);
    return (c & 0x80) ? -v : v;
}

static inline float vox_kv8_round_(float x) { return vox_kv8_decode_(vox_kv8_encode_(x)); }

#endif
