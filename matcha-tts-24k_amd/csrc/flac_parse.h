// FLAC in: the parser of include/mtts.h "FLAC in", compiled for the host and for the device.
//
// Plain functions over a byte pointer and a byte count, no HIP calls: the bit reader, the metadata walk, the frame-header parse with
// its CRC-8 (the candidate rule), the subframe parse (Rice partitions, escapes, warm-up samples, LPC coefficients), the prediction
// restore, and the acceptance walk of a whole stream (parse_stream: what mtts_flac_parse_host and tools/flac_parse_check.cpp run;
// the kernels of flac_decode.hip run the same header, frame and stereo functions and restate the walk over their candidate lists).
//
// Safety is decided in the bit reader: every read is bounded by the byte count, a read past the end returns zeros and sets the
// sticky `overrun`, and a unary run is counted with clz on a refilled 64-bit window and stops at the end of the row.  No loop's trip
// count comes from the stream without a bound: samples <= the block size (<= max_block <= 4608), coefficients <= 32, partitions
// <= the block size, metadata blocks and unary refills <= the row's bytes / 4.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FLAC_HD __host__ __device__ inline
#else
#define FLAC_HD inline
#endif

namespace mtts_flac {

constexpr int MAX_BLOCK = 4608;        // the streamable subset's limit at <= 48 kHz
constexpr int MIN_MAX_BLOCK = 16;
constexpr int MAX_ORDER = 32;
constexpr int MAX_HEADER = 16;         // sync 2, codes 2, coded number 7, block-size tail 2, rate tail 2, CRC-8 1
constexpr int STREAM_HEAD = 42;        // "fLaC", a block header, STREAMINFO

struct Info {                          // what the metadata chain says
    int32_t ok, min_bs, max_bs, rate, channels, bps;
    int64_t total, first;              // samples per channel (0: unknown); the first byte behind the metadata
};
struct Header {                        // a candidate's frame header
    int32_t variable, bs, assign, nbytes;   // blocking strategy bit, samples, channel assignment 0..10, header bytes with the CRC-8
    int64_t number;                    // the coded number: a frame number (fixed) or the first sample's number (variable)
};

FLAC_HD uint32_t crc8_byte(uint32_t c, uint32_t byte) {
    c ^= byte;
    for (int i = 0; i < 8; ++i) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
    return c;
}
FLAC_HD uint32_t crc16_mulx(uint32_t p) { return (p & 0x8000u) ? ((p << 1) ^ 0x8005u) & 0xFFFFu : p << 1; }
FLAC_HD uint32_t crc16_byte(uint32_t c, uint32_t byte) {
    c ^= byte << 8;
    for (int i = 0; i < 8; ++i) c = crc16_mulx(c);
    return c;
}
FLAC_HD uint32_t crc16_mul(uint32_t x, uint32_t y) {         // x * y mod the polynomial (bit i = the coefficient of x^i)
    uint32_t r = 0;
    for (int i = 15; i >= 0; --i) {
        r = crc16_mulx(r);
        if ((y >> i) & 1u) r ^= x;
    }
    return r;
}
FLAC_HD uint32_t crc16_xpow(uint64_t e) {                    // x^e mod the polynomial, by squaring: at most 64 steps
    uint32_t r = 1, base = 2;
    for (int i = 0; i < 64 && e; ++i, e >>= 1) {
        if (e & 1) r = crc16_mul(r, base);
        base = crc16_mul(base, base);
    }
    return r;
}

// ------------------------------------------------------------------------------------------------ the bit reader
struct Bits {
    const uint8_t* p;
    int64_t n, next, pos;              // bytes of the row; the next byte to load; the bit position of the next read
    uint64_t buf;                      // `have` valid bits from the top, zeros below
    int have, overrun;
};
FLAC_HD void bits_init(Bits& r, const uint8_t* p, int64_t n, int64_t at) {
    r.p = p; r.n = n; r.next = at; r.pos = 8 * at; r.buf = 0; r.have = 0; r.overrun = 0;
}
FLAC_HD void bits_refill(Bits& r) {                          // afterwards 32 <= have <= 63; bytes at or beyond n read as zeros
    if (r.have < 32) {
        uint32_t w = 0;
        if (r.next + 4 <= r.n) {
            __builtin_memcpy(&w, r.p + r.next, 4);
            w = __builtin_bswap32(w);
        } else {
            for (int j = 0; j < 4; ++j)
                if (r.next + j < r.n) w |= (uint32_t)r.p[r.next + j] << (24 - 8 * j);
        }
        r.buf |= (uint64_t)w << (32 - r.have);
        r.have += 32;
        r.next += 4;
    }
}
FLAC_HD uint32_t bits_read(Bits& r, int nb) {                // nb in [0, 32]
    bits_refill(r);
    const uint32_t v = nb ? (uint32_t)(r.buf >> (64 - nb)) : 0u;
    r.buf <<= nb;
    r.have -= nb;
    r.pos += nb;
    if (r.pos > 8 * r.n) { r.overrun = 1; return 0u; }
    return v;
}
FLAC_HD int32_t bits_signed(Bits& r, int nb) {               // two's complement in nb bits, nb in [0, 32]
    const uint32_t v = bits_read(r, nb);
    if (nb == 0) return 0;
    return (int32_t)(v << (32 - nb)) >> (32 - nb);
}
FLAC_HD uint64_t bits_unary(Bits& r) {                       // zero bits ahead of the next one bit, which is consumed
    uint64_t count = 0;
    for (;;) {                                               // (each pass consumes >= 32 bits or returns)
        bits_refill(r);
        if (r.buf == 0) {
            count += r.have;
            r.pos += r.have;
            r.have = 0;
            if (r.pos >= 8 * r.n) { r.overrun = 1; return count; }
            continue;
        }
        const int z = __builtin_clzll(r.buf);                // z < have <= 63
        r.buf <<= z + 1;
        r.have -= z + 1;
        r.pos += z + 1;
        return count + z;
    }
}

// ------------------------------------------------------------------------------------------------ the metadata chain
// "fLaC", STREAMINFO first, then any chain of blocks skipped by their lengths.  false: the row is refused.
FLAC_HD bool parse_info(const uint8_t* p, int64_t n, int max_block, Info& info) {
    info.ok = 0; info.min_bs = info.max_bs = info.rate = info.channels = info.bps = 0; info.total = 0; info.first = 0;
    if (n < STREAM_HEAD || p[0] != 0x66 || p[1] != 0x4C || p[2] != 0x61 || p[3] != 0x43) return false;
    int64_t at = 4;
    for (int64_t blocks = 0; blocks <= n / 4; ++blocks) {
        if (at + 4 > n) return false;
        const int last = p[at] >> 7, type = p[at] & 0x7F;
        const int64_t len = (int64_t)p[at + 1] << 16 | (int64_t)p[at + 2] << 8 | p[at + 3];
        if (type == 127 || (blocks == 0) != (type == 0) || at + 4 + len > n) return false;
        if (type == 0) {
            if (len != 34) return false;
            const uint8_t* s = p + at + 4;
            info.min_bs = s[0] << 8 | s[1];
            info.max_bs = s[2] << 8 | s[3];
            info.rate = s[10] << 12 | s[11] << 4 | s[12] >> 4;
            info.channels = ((s[12] >> 1) & 7) + 1;
            info.bps = ((s[12] & 1) << 4 | s[13] >> 4) + 1;
            info.total = (int64_t)(s[13] & 15) << 32 | (int64_t)s[14] << 24 | (int64_t)s[15] << 16 | (int64_t)s[16] << 8 | s[17];
        }
        at += 4 + len;
        if (last) {
            if (info.bps < 8 || info.bps > 24 || info.rate < 1 || info.min_bs < 16 || info.min_bs > info.max_bs || info.max_bs > max_block)
                return false;
            info.first = at;
            info.ok = 1;
            return true;
        }
    }
    return false;
}

// ------------------------------------------------------------------------------------------------ the candidate rule
// Whether the bytes at `at` are a frame header that agrees with STREAMINFO and whose CRC-8 matches.  Reads [at, at + 16) at most,
// and nothing at or beyond n.
FLAC_HD bool parse_header(const uint8_t* p, int64_t n, int64_t at, const Info& info, Header& h) {
    if (at < 0 || at + 6 > n || p[at] != 0xFF || (p[at + 1] & 0xFE) != 0xF8) return false;
    h.variable = p[at + 1] & 1;
    const int bcode = p[at + 2] >> 4, rcode = p[at + 2] & 15, assign = p[at + 3] >> 4, scode = (p[at + 3] >> 1) & 7;
    if ((p[at + 3] & 1) || bcode == 0 || rcode == 15 || assign > 10 || scode == 3) return false;
    int64_t i = at + 4;
    const uint32_t lead = p[i++];
    int extra = 0;
    if (lead >= 0x80) {
        if (lead < 0xC0 || lead == 0xFF) return false;
        extra = __builtin_clz(~(lead << 24)) - 1;            // leading ones - 1: 1..6
    }
    uint64_t number = extra ? (lead & (0x7Fu >> (extra + 1))) : lead;
    if (i + extra > n) return false;
    for (int j = 0; j < extra; ++j) {
        const uint32_t c = p[i++];
        if ((c & 0xC0u) != 0x80u) return false;
        number = number << 6 | (c & 63u);
    }
    h.number = (int64_t)number;
    int bs;
    if (bcode == 1) bs = 192;
    else if (bcode <= 5) bs = 144 << bcode;
    else if (bcode == 6) { if (i + 1 > n) return false; bs = p[i] + 1; i += 1; }
    else if (bcode == 7) { if (i + 2 > n) return false; bs = (p[i] << 8 | p[i + 1]) + 1; i += 2; }
    else bs = 1 << bcode;
    int rate = info.rate;
    switch (rcode) {
        case 0: break;
        case 1: rate = 88200; break;   case 2: rate = 176400; break;  case 3: rate = 192000; break;  case 4: rate = 8000; break;
        case 5: rate = 16000; break;   case 6: rate = 22050; break;   case 7: rate = 24000; break;   case 8: rate = 32000; break;
        case 9: rate = 44100; break;   case 10: rate = 48000; break;  case 11: rate = 96000; break;
        case 12: if (i + 1 > n) return false; rate = p[i] * 1000; i += 1; break;
        default: if (i + 2 > n) return false; rate = (p[i] << 8 | p[i + 1]) * (rcode == 14 ? 10 : 1); i += 2; break;
    }
    const int bps = scode == 0 ? info.bps : scode == 1 ? 8 : scode == 2 ? 12 : scode == 4 ? 16 : scode == 5 ? 20 : scode == 6 ? 24 : 32;
    if (i + 1 > n) return false;
    uint32_t crc = 0;
    for (int64_t j = at; j < i; ++j) crc = crc8_byte(crc, p[j]);   // (at most 15 bytes)
    if (crc != p[i]) return false;
    if (rate != info.rate || bps != info.bps || (assign < 8 ? assign + 1 : 2) != info.channels || bs > info.max_bs) return false;
    h.bs = bs;
    h.assign = assign;
    h.nbytes = (int32_t)(i + 1 - at);
    return true;
}

// ------------------------------------------------------------------------------------------------ subframes
// The residual of n - order samples into out[order, n) (parsed for its length only when out is null).  -1: refused.
FLAC_HD int parse_residual(Bits& r, int n, int order, int32_t* out) {
    const uint32_t method = bits_read(r, 2);
    if (method > 1) return -1;
    const int pbits = 4 + (int)method;
    const int po = (int)bits_read(r, 4);
    if ((n & ((1 << po) - 1)) || (n >> po) < order) return -1;   // (so 2^po <= n: the partition loop is bounded by the block)
    const int psize = n >> po;
    int i = order;
    for (int p = 0; p < (1 << po); ++p) {
        const int cnt = psize - (p == 0 ? order : 0);
        const int k = (int)bits_read(r, pbits);
        if (r.overrun) return -1;
        if (k == (1 << pbits) - 1) {                         // escape: raw two's-complement words of 0..31 bits
            const int raw = (int)bits_read(r, 5);
            for (int j = 0; j < cnt; ++j, ++i) {
                const int32_t v = bits_signed(r, raw);
                if (r.overrun) return -1;
                if (out) out[i] = v;
            }
        } else {
            for (int j = 0; j < cnt; ++j, ++i) {
                const uint64_t q = bits_unary(r);
                const uint32_t low = bits_read(r, k);
                if (r.overrun || q >= (1ull << (32 - k))) return -1;
                const uint32_t u = (uint32_t)(q << k) | low;
                if (u == 0xFFFFFFFFu) return -1;             // -2^31: outside what a residual may be
                if (out) out[i] = (int32_t)(u >> 1) ^ -(int32_t)(u & 1u);
            }
        }
    }
    return 0;
}

// Samples from residuals, in place: out[0, order) are the warm-up samples, out[order, n) the residuals.  Sums are int64 (25-bit
// samples, 15-bit coefficients and 32 taps need 45 bits); a sample is the low 32 bits of residual + prediction.
FLAC_HD void restore_fixed(int32_t* out, int n, int order) {
    for (int i = order; i < n; ++i) {
        const uint32_t x1 = i >= 1 ? (uint32_t)out[i - 1] : 0u, x2 = i >= 2 ? (uint32_t)out[i - 2] : 0u;
        const uint32_t x3 = i >= 3 ? (uint32_t)out[i - 3] : 0u, x4 = i >= 4 ? (uint32_t)out[i - 4] : 0u;
        uint32_t pred = 0;
        if (order == 1) pred = x1;
        else if (order == 2) pred = 2u * x1 - x2;
        else if (order == 3) pred = 3u * x1 - 3u * x2 + x3;
        else if (order == 4) pred = 4u * x1 - 6u * x2 + 4u * x3 - x4;
        out[i] = (int32_t)((uint32_t)out[i] + pred);
    }
}
FLAC_HD void restore_lpc(int32_t* out, int n, int order, const int32_t* coef, int shift) {
    for (int i = order; i < n; ++i) {
        int64_t sum = 0;
        for (int j = 0; j < order; ++j) sum += (int64_t)coef[j] * out[i - 1 - j];
        out[i] = (int32_t)((uint32_t)out[i] + (uint32_t)(uint64_t)(sum >> shift));
    }
}

// One subframe of n samples of bps bits (a side channel: bps + 1) into out[0, n), or parsed for its length only (out null).
// coef: 32 words of scratch.  -1: refused.
FLAC_HD int parse_subframe(Bits& r, int n, int bps, int32_t* out, int32_t* coef) {
    if (bits_read(r, 1)) return -1;
    const int type = (int)bits_read(r, 6);
    int wasted = 0;
    if (bits_read(r, 1)) {
        const uint64_t w = bits_unary(r);
        if (r.overrun || w + 2 > (uint64_t)bps) return -1;   // at least one bit is left
        wasted = (int)w + 1;
    }
    const int eff = bps - wasted;
    if (type == 0) {
        const int32_t v = bits_signed(r, eff);
        if (out) for (int i = 0; i < n; ++i) out[i] = v;
    } else if (type == 1) {
        for (int i = 0; i < n; ++i) {
            const int32_t v = bits_signed(r, eff);
            if (r.overrun) return -1;
            if (out) out[i] = v;
        }
    } else {
        const bool lpc = type >= 32;
        if (!lpc && (type < 8 || type > 12)) return -1;      // reserved types
        const int order = lpc ? type - 31 : type - 8;
        if (order > n) return -1;
        for (int i = 0; i < order; ++i) {
            const int32_t v = bits_signed(r, eff);
            if (out) out[i] = v;
        }
        int shift = 0;
        if (lpc) {
            const int prec = (int)bits_read(r, 4);
            if (prec == 15) return -1;
            shift = bits_signed(r, 5);
            if (shift < 0) return -1;
            for (int j = 0; j < order; ++j) coef[j] = bits_signed(r, prec + 1);
        }
        if (r.overrun || parse_residual(r, n, order, out)) return -1;
        if (out) {
            if (lpc) restore_lpc(out, n, order, coef, shift);
            else restore_fixed(out, n, order);
        }
    }
    if (r.overrun) return -1;
    if (out && wasted) for (int i = 0; i < n; ++i) out[i] = (int32_t)((uint32_t)out[i] << wasted);
    return 0;
}

// The subframes of the candidate at `at` (header h): the first channel's samples to ch0[0, bs); for side/right and mid/side the
// second's to ch1[0, bs) (left/side needs only the left).  Further channels are parsed for their length.  Returns the frame's byte
// length with its CRC-16, which is not checked here, or -1 when the subframes do not parse inside the row.
FLAC_HD int64_t parse_frame(const uint8_t* p, int64_t n, int64_t at, const Header& h, int bps, int32_t* ch0, int32_t* ch1, int32_t* coef) {
    Bits r;
    bits_init(r, p, n, at + h.nbytes);
    const int nch = h.assign < 8 ? h.assign + 1 : 2;
    for (int c = 0; c < nch; ++c) {
        const bool side = (h.assign == 8 && c == 1) || (h.assign == 9 && c == 0) || (h.assign == 10 && c == 1);
        int32_t* dst = c == 0 ? ch0 : (c == 1 && h.assign >= 9) ? ch1 : nullptr;
        if (parse_subframe(r, h.bs, bps + (side ? 1 : 0), dst, coef)) return -1;
    }
    bits_read(r, (int)((8 - (r.pos & 7)) & 7));               // to the byte boundary (the padding bits are not looked at)
    const int64_t end = r.pos >> 3;
    if (r.overrun || end + 2 > n) return -1;
    return end + 2 - at;
}

// Channel 0 of a frame from its first two coded channels
FLAC_HD int32_t first_channel(int assign, int32_t a, int32_t b) {
    if (assign == 9) return (int32_t)((uint32_t)a + (uint32_t)b);                  // side + right
    if (assign == 10) return (int32_t)((((int64_t)a * 2 | (b & 1)) + b) >> 1);     // mid, side
    return a;
}
FLAC_HD bool in_range(int32_t v, int bps) { return v >= -(1 << (bps - 1)) && v < (1 << (bps - 1)); }

// ------------------------------------------------------------------------------------------------ the acceptance walk
// State of the walk over the frames of a row; the host walk below and flac_walk_kernel step it the same way.
struct Walk {
    int64_t total, frames;
    int32_t variable, bs0, short_seen;
};
FLAC_HD void walk_init(Walk& w) { w.total = 0; w.frames = 0; w.variable = 0; w.bs0 = 0; w.short_seen = 0; }
// Whether a frame with this header may come next; advances the state when it may.
FLAC_HD bool walk_step(Walk& w, int variable, int bs, int64_t number) {
    if (w.frames == 0) { w.variable = variable; w.bs0 = bs; }
    else if (variable != w.variable) return false;
    if (w.variable) {
        if (number != w.total) return false;
    } else {
        if (number != w.frames || w.short_seen || bs > w.bs0) return false;
        if (bs < w.bs0) w.short_seen = 1;
    }
    w.total += bs;
    w.frames += 1;
    return true;
}
FLAC_HD int64_t walk_verdict(const Walk& w, const Info& info, int64_t capacity) {
    if (info.total == 0) return w.frames == 0 ? 0 : -1;      // an empty clip; an unknown length with frames is refused
    return (w.total == info.total && w.total <= capacity) ? w.total : -1;
}

// A whole stream on the host side of the contract: channel 0's samples to out[0, capacity).  ch1: max_block words of scratch.
// Returns the sample count or -1; info is filled whenever the metadata parsed.
FLAC_HD int64_t parse_stream(const uint8_t* p, int64_t n, int max_block, int32_t* out, int64_t capacity, int32_t* ch1, Info& info) {
    if (n < 0 || max_block < MIN_MAX_BLOCK || max_block > MAX_BLOCK || !parse_info(p, n, max_block, info)) return -1;
    int32_t coef[MAX_ORDER];
    Walk w;
    walk_init(w);
    int64_t at = info.first;
    while (at < n) {                                         // (a frame is at least 9 bytes: at most n / 9 passes)
        Header h;
        if (!parse_header(p, n, at, info, h)) return -1;
        const int64_t before = w.total;
        if (!walk_step(w, h.variable, h.bs, h.number) || w.total > capacity) return -1;
        int32_t* ch0 = out + before;
        const int64_t len = parse_frame(p, n, at, h, info.bps, ch0, ch1, coef);
        if (len < 0) return -1;
        uint32_t crc = 0;
        for (int64_t j = at; j < at + len - 2; ++j) crc = crc16_byte(crc, p[j]);
        if (crc != ((uint32_t)p[at + len - 2] << 8 | p[at + len - 1])) return -1;
        for (int i = 0; i < h.bs; ++i) {
            const int32_t v = first_channel(h.assign, ch0[i], h.assign >= 9 ? ch1[i] : 0);
            if (!in_range(v, info.bps)) return -1;
            ch0[i] = v;
        }
        at += len;
    }
    return walk_verdict(w, info, capacity);
}

}  // namespace mtts_flac
