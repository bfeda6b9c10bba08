// JPEG decode split between host and device (include/poseadv.h: pa_jpeg_*).
//   host  : marker parse + baseline Huffman decode of the one interleaved scan -> int16 coefficient planes (pure C++, no HIP call,
//           no global state: callable from many threads and on a machine without a GPU)
//   device: (a) dequantise + 8x8 inverse DCT (libjpeg's jidctint) + range limit -> uint8 component planes in the caller's workspace
//           (b) "fancy" chroma upsampling (jdsample) + YCbCr -> RGB (jdcolor) + zero padding -> frames [B][Hs][Ws][3], sizes [B][2]
// All integer arithmetic, byte-exact with libjpeg / libjpeg-turbo (what Pillow decodes with).
#include "../../include/poseadv.h"
#include "common.h"
#include <stdio.h>
#include <string.h>

// ------------------------------------------------------------------------------------------------ host: parse + entropy decode
namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

enum { LOOK_BITS = 9 };

struct HuffTable {
    bool defined = false;
    uint8_t counts[17];
    uint8_t symbols[256];
    uint16_t look[1 << LOOK_BITS];      // (length << 8) | symbol for codes of <= LOOK_BITS bits, 0 otherwise
    int16_t fast_ac[1 << LOOK_BITS];    // AC tables: (value << 8) | (run << 4) | (code + value bits) where both fit LOOK_BITS, 0 otherwise
    int32_t maxcode[18];                // largest code of each length (-1: none); [17] = sentinel
    int32_t valoff[17];                 // symbols index of the first code of a length minus that code
};

// canonical code of a DHT segment; false when the counts do not form a prefix code
bool build_table(HuffTable& t) {
    int code = 0, k = 0;
    memset(t.look, 0, sizeof t.look);
    for (int len = 1; len <= 16; ++len) {
        t.valoff[len] = k - code;
        if (t.counts[len]) {
            if (code + t.counts[len] > (1 << len)) return false;
            for (int i = 0; i < t.counts[len]; ++i, ++k, ++code) {
                if (len <= LOOK_BITS) {
                    int first = code << (LOOK_BITS - len), cnt = 1 << (LOOK_BITS - len);
                    for (int j = 0; j < cnt; ++j) t.look[first + j] = (uint16_t)((len << 8) | t.symbols[k]);
                }
            }
            t.maxcode[len] = code - 1;
        } else {
            t.maxcode[len] = -1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    for (int idx = 0; idx < (1 << LOOK_BITS); ++idx) {
        t.fast_ac[idx] = 0;
        unsigned e = t.look[idx];
        int len = e >> 8, run = (e >> 4) & 15, sz = e & 15;
        if (e && sz && len + sz <= LOOK_BITS) {
            int bits = (idx >> (LOOK_BITS - len - sz)) & ((1 << sz) - 1);
            int v = bits < (1 << (sz - 1)) ? bits - (1 << sz) + 1 : bits;
            if (v >= -128 && v <= 127) t.fast_ac[idx] = (int16_t)(v * 256 + run * 16 + len + sz);
        }
    }
    t.defined = true;
    return true;
}

struct Header {
    int width = 0, height = 0, ncomp = 0, restart = 0;
    int id[4], h[4], v[4], tq[4], td[4], ta[4];
    bool quant_defined[4] = {false, false, false, false};
    uint16_t quant[4][64];              // natural order
    HuffTable dc[4], ac[4];
    bool jfif = false, adobe = false;
    int adobe_transform = 0;
    size_t scan_at = 0;                 // first byte of the entropy-coded data
};

int fail(int code, const char* msg) { pa_set_error_msg(msg); return code; }

inline bool is_sof(int m) { return m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC; }

// markers up to and including SOS; every read is bounds-checked against n
int parse_header(const uint8_t* d, size_t n, Header& hd, bool need_tables) {
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(PA_JPEG_CORRUPT, "jpeg: no SOI marker");
    size_t p = 2;
    bool have_sof = false;
    for (;;) {
        while (p < n && d[p] != 0xFF) ++p;                       // (garbage between segments is skipped, as libjpeg does)
        while (p < n && d[p] == 0xFF) ++p;                       // fill bytes
        if (p >= n) return fail(PA_JPEG_CORRUPT, "jpeg: truncated before the scan");
        int m = d[p++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // no payload
        if (m == 0xD9) return fail(PA_JPEG_CORRUPT, "jpeg: EOI before any scan");
        if (m == 0xD8) return fail(PA_JPEG_CORRUPT, "jpeg: second SOI");
        if (p + 2 > n) return fail(PA_JPEG_CORRUPT, "jpeg: truncated segment length");
        size_t len = ((size_t)d[p] << 8) | d[p + 1];
        if (len < 2 || p + len > n) return fail(PA_JPEG_CORRUPT, "jpeg: segment runs past the end of the data");
        const uint8_t* s = d + p + 2;
        size_t sl = len - 2;
        if (is_sof(m)) {
            if (have_sof) return fail(PA_JPEG_CORRUPT, "jpeg: second frame header");
            if (m != 0xC0 && m != 0xC1) return fail(PA_JPEG_UNSUPPORTED, "jpeg: progressive, lossless, hierarchical or arithmetic coding");
            if (sl < 6) return fail(PA_JPEG_CORRUPT, "jpeg: short frame header");
            int prec = s[0];
            hd.height = (s[1] << 8) | s[2];
            hd.width = (s[3] << 8) | s[4];
            hd.ncomp = s[5];
            if (prec == 12) return fail(PA_JPEG_UNSUPPORTED, "jpeg: 12-bit samples");
            if (prec != 8) return fail(PA_JPEG_CORRUPT, "jpeg: bad sample precision");
            if (hd.width == 0 || hd.height == 0) return fail(PA_JPEG_CORRUPT, "jpeg: empty image (or DNL-defined height)");
            if (hd.ncomp < 1 || hd.ncomp > 4 || sl < (size_t)(6 + 3 * hd.ncomp)) return fail(PA_JPEG_CORRUPT, "jpeg: bad component count");
            for (int i = 0; i < hd.ncomp; ++i) {
                hd.id[i] = s[6 + 3 * i];
                hd.h[i] = s[7 + 3 * i] >> 4;
                hd.v[i] = s[7 + 3 * i] & 15;
                hd.tq[i] = s[8 + 3 * i];
                if (hd.h[i] < 1 || hd.h[i] > 4 || hd.v[i] < 1 || hd.v[i] > 4 || hd.tq[i] > 3) return fail(PA_JPEG_CORRUPT, "jpeg: bad component in the frame header");
            }
            have_sof = true;
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < sl) {
                if (q + 17 > sl) return fail(PA_JPEG_CORRUPT, "jpeg: short DHT");
                int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return fail(PA_JPEG_CORRUPT, "jpeg: bad Huffman table id");
                HuffTable& t = tc ? hd.ac[th] : hd.dc[th];
                int total = 0;
                t.counts[0] = 0;
                for (int i = 1; i <= 16; ++i) { t.counts[i] = s[q + i]; total += s[q + i]; }
                if (total > 256 || q + 17 + total > sl) return fail(PA_JPEG_CORRUPT, "jpeg: bad DHT counts");
                memcpy(t.symbols, s + q + 17, total);
                t.defined = false;
                if (need_tables && !build_table(t)) return fail(PA_JPEG_CORRUPT, "jpeg: DHT is not a prefix code");
                if (!need_tables) t.defined = true;
                q += 17 + total;
            }
        } else if (m == 0xDB) {
            size_t q = 0;
            while (q < sl) {
                int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq > 1 || tq > 3) return fail(PA_JPEG_CORRUPT, "jpeg: bad quantisation table id");
                size_t need = pq ? 128 : 64;
                if (q + 1 + need > sl) return fail(PA_JPEG_CORRUPT, "jpeg: short DQT");
                for (int i = 0; i < 64; ++i)
                    hd.quant[tq][kZigzag[i]] = pq ? (uint16_t)((s[q + 1 + 2 * i] << 8) | s[q + 2 + 2 * i]) : s[q + 1 + i];
                hd.quant_defined[tq] = true;
                q += 1 + need;
            }
        } else if (m == 0xDD) {
            if (sl < 2) return fail(PA_JPEG_CORRUPT, "jpeg: short DRI");
            hd.restart = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {
            if (sl >= 5 && !memcmp(s, "JFIF\0", 5)) hd.jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) { hd.adobe = true; hd.adobe_transform = s[11]; }
        } else if (m == 0xDA) {
            if (!have_sof) return fail(PA_JPEG_CORRUPT, "jpeg: scan before the frame header");
            if (sl < 1) return fail(PA_JPEG_CORRUPT, "jpeg: short SOS");
            int ns = s[0];
            if (ns < 1 || ns > 4 || sl < (size_t)(4 + 2 * ns)) return fail(PA_JPEG_CORRUPT, "jpeg: bad SOS");
            if (ns != hd.ncomp) return fail(PA_JPEG_UNSUPPORTED, "jpeg: several scans");
            for (int i = 0; i < ns; ++i) {
                if (s[1 + 2 * i] != hd.id[i]) return fail(PA_JPEG_UNSUPPORTED, "jpeg: scan components out of frame order");
                hd.td[i] = s[2 + 2 * i] >> 4;
                hd.ta[i] = s[2 + 2 * i] & 15;
                if (hd.td[i] > 3 || hd.ta[i] > 3) return fail(PA_JPEG_CORRUPT, "jpeg: bad table selector in SOS");
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return fail(PA_JPEG_CORRUPT, "jpeg: bad spectral selection in a sequential scan");
            hd.scan_at = p + len;
            return 0;
        }
        p += len;
    }
}

// Header -> descriptor (and the colour-space / sampling rules of the supported set)
int describe(const Header& hd, pa_jpeg_desc* desc) {
    memset(desc, 0, sizeof *desc);
    if (hd.ncomp != 1 && hd.ncomp != 3) return fail(PA_JPEG_UNSUPPORTED, "jpeg: CMYK / YCCK or a two-component file");
    if (hd.ncomp == 3) {
        bool rgb_ids = hd.id[0] == 'R' && hd.id[1] == 'G' && hd.id[2] == 'B';
        bool ycc = hd.jfif ? true : hd.adobe ? hd.adobe_transform != 0 : !rgb_ids;       // jdapimin.c default_decompress_parms
        if (!ycc) return fail(PA_JPEG_UNSUPPORTED, "jpeg: RGB colour space");
        bool ok = hd.h[1] == 1 && hd.v[1] == 1 && hd.h[2] == 1 && hd.v[2] == 1 &&
                  ((hd.h[0] == 1 && hd.v[0] == 1) || (hd.h[0] == 2 && hd.v[0] == 1) || (hd.h[0] == 2 && hd.v[0] == 2));
        if (!ok) return fail(PA_JPEG_UNSUPPORTED, "jpeg: sampling factors other than 4:4:4, 4:2:2, 4:2:0");
        // libjpeg takes its triangle upsampler only for a component wider than 2 samples (jdsample.c) and replicates otherwise
        if (hd.h[0] == 2 && (hd.width + 1) / 2 <= 2) return fail(PA_JPEG_UNSUPPORTED, "jpeg: subsampled component narrower than 3 samples");
    }
    desc->width = hd.width;
    desc->height = hd.height;
    desc->ncomp = hd.ncomp;
    desc->restart_interval = hd.restart;
    int hmax = hd.ncomp == 1 ? 1 : hd.h[0], vmax = hd.ncomp == 1 ? 1 : hd.v[0];
    int mcus_w = (hd.width + 8 * hmax - 1) / (8 * hmax), mcus_h = (hd.height + 8 * vmax - 1) / (8 * vmax);
    int64_t off = 0;
    for (int i = 0; i < hd.ncomp; ++i) {
        pa_jpeg_comp& c = desc->comp[i];
        c.h = hd.ncomp == 1 ? 1 : hd.h[i];
        c.v = hd.ncomp == 1 ? 1 : hd.v[i];
        c.bw = mcus_w * c.h;
        c.bh = mcus_h * c.v;
        c.offset = off;
        off += (int64_t)c.bw * c.bh * 64;
        if (!hd.quant_defined[hd.tq[i]]) return fail(PA_JPEG_CORRUPT, "jpeg: a component names a quantisation table that was not defined");
        memcpy(desc->quant[i], hd.quant[hd.tq[i]], sizeof desc->quant[i]);
    }
    desc->total_elems = off;
    return 0;
}

// MSB-first bit reader over the entropy-coded segment: removes stuffed zero bytes, stops in front of a marker (and at the end of the
// data) and feeds zero bits from there on; `phantom` counts those, so that a decoder that consumed one knows the data ended early.
struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf = 0;      // the next bits are at the top
    int cnt = 0;           // valid bits in buf
    int phantom = 0;       // zero bits appended after the stop
    bool stopped = false;

    inline void fill() {
        while (cnt <= 56) {
            unsigned b = 0;
            if (!stopped) {
                if (p + 4 <= end && cnt <= 32) {            // four plain bytes at once
                    uint32_t w;
                    memcpy(&w, p, 4);
                    if (!has_ff(w)) {
                        w = __builtin_bswap32(w);
                        buf |= (uint64_t)w << (32 - cnt);
                        cnt += 32;
                        p += 4;
                        continue;
                    }
                }
                if (p >= end) {
                    stopped = true;
                } else {
                    b = *p;
                    if (b == 0xFF) {
                        if (p + 1 < end && p[1] == 0x00) p += 2;
                        else { stopped = true; b = 0; }
                    } else {
                        ++p;
                    }
                }
            }
            if (stopped) phantom += 8;
            buf |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    static inline bool has_ff(uint32_t w) { return (w & 0xFF) == 0xFF || (w & 0xFF00) == 0xFF00 || (w & 0xFF0000) == 0xFF0000 || (w >> 24) == 0xFF; }
    inline unsigned peek(int nbits) const { return (unsigned)(buf >> (64 - nbits)); }
    inline void skip(int nbits) { buf <<= nbits; cnt -= nbits; }
    inline bool overrun() const { return phantom > cnt; }       // some consumed bit was not in the data
    void reset() { buf = 0; cnt = 0; phantom = 0; stopped = false; }
};

// one Huffman symbol; -1 for a code that is in no table (needs >= 16 valid bits in the reader)
inline int decode_symbol(BitReader& br, const HuffTable& t) {
    unsigned e = t.look[br.peek(LOOK_BITS)];
    if (e) { br.skip(e >> 8); return e & 255; }
    unsigned code16 = br.peek(16);
    for (int len = LOOK_BITS + 1; len <= 16; ++len) {
        int code = (int)(code16 >> (16 - len));
        if (code <= t.maxcode[len]) {
            br.skip(len);
            return t.symbols[(code + t.valoff[len]) & 255];
        }
    }
    return -1;
}

inline int extend(unsigned bits, int s) { return bits < (1u << (s - 1)) ? (int)bits - (1 << s) + 1 : (int)bits; }

inline int decode_block(BitReader& br, const HuffTable& dc, const HuffTable& ac, int& pred, int16_t* blk) {
    memset(blk, 0, 64 * sizeof(int16_t));
    if (br.cnt < 32) br.fill();                      // a symbol and its extra bits take at most 32
    int s = decode_symbol(br, dc);
    if (s < 0 || s > 16) return 1;
    if (s) { pred += extend(br.peek(s), s); br.skip(s); }
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        if (br.cnt < 32) br.fill();
        int f = ac.fast_ac[br.peek(LOOK_BITS)];
        if (f) {                                     // short code + small value: one lookup
            k += (f >> 4) & 15;
            if (k > 63) return 1;
            blk[kZigzag[k]] = (int16_t)(f >> 8);
            br.skip(f & 15);
            ++k;
            continue;
        }
        int rs = decode_symbol(br, ac);
        if (rs < 0) return 1;
        int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return 1;
        blk[kZigzag[k]] = (int16_t)extend(br.peek(s), s);
        br.skip(s);
        ++k;
    }
    return 0;
}

int entropy_decode(const uint8_t* d, size_t n, const Header& hd, const pa_jpeg_desc& desc, int16_t* coef) {
    for (int i = 0; i < hd.ncomp; ++i)
        if (!hd.dc[hd.td[i]].defined || !hd.ac[hd.ta[i]].defined) return fail(PA_JPEG_CORRUPT, "jpeg: the scan names a Huffman table that was not defined");
    BitReader br;
    br.p = d + hd.scan_at;
    br.end = d + n;
    int pred[3] = {0, 0, 0};
    const int ncomp = hd.ncomp;
    const int hmax = desc.comp[0].h, vmax = desc.comp[0].v;
    const int mcus_w = desc.comp[0].bw / hmax, mcus_h = desc.comp[0].bh / vmax;
    int to_restart = hd.restart, next_rst = 0;
    for (int my = 0; my < mcus_h; ++my) {
        for (int mx = 0; mx < mcus_w; ++mx) {
            if (hd.restart && to_restart == 0) {
                // byte-align: what is left in the reader is padding.  The reader refills lazily (below 32 bits), so it may not have
                // met the marker yet when the interval's last symbol left it fewer than 8 bits: drop those and look
                if (!br.stopped) {
                    br.skip(br.cnt & 7);
                    if (br.cnt == 0) br.fill();
                }
                if (!br.stopped || br.cnt - br.phantom >= 8) return fail(PA_JPEG_CORRUPT, "jpeg: entropy data where a restart marker was expected");
                const uint8_t* q = br.p;
                while (q < br.end && *q == 0xFF) ++q;
                if (q >= br.end || q == br.p || *q != 0xD0 + next_rst) return fail(PA_JPEG_CORRUPT, "jpeg: missing or out-of-order restart marker");
                br.p = q + 1;
                br.reset();
                next_rst = (next_rst + 1) & 7;
                to_restart = hd.restart;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int i = 0; i < ncomp; ++i) {
                const pa_jpeg_comp& c = desc.comp[i];
                const HuffTable& dc = hd.dc[hd.td[i]];
                const HuffTable& ac = hd.ac[hd.ta[i]];
                for (int by = 0; by < c.v; ++by)
                    for (int bx = 0; bx < c.h; ++bx) {
                        int64_t blk = (int64_t)(my * c.v + by) * c.bw + (mx * c.h + bx);
                        if (decode_block(br, dc, ac, pred[i], coef + c.offset + blk * 64)) return fail(PA_JPEG_CORRUPT, "jpeg: bad Huffman code in the scan");
                    }
            }
            if (br.overrun()) return fail(PA_JPEG_CORRUPT, "jpeg: the entropy-coded data ends early");
            --to_restart;
        }
    }
    return 0;
}

}  // namespace

extern "C" int pa_jpeg_info_host(const uint8_t* data, size_t n, pa_jpeg_desc* desc) {
    if (!data || !desc) return fail(1, "pa_jpeg_info_host: NULL argument");
    Header hd;
    int rc = parse_header(data, n, hd, false);
    if (rc) { memset(desc, 0, sizeof *desc); return rc; }
    return describe(hd, desc);
}

extern "C" int pa_jpeg_entropy_host(const uint8_t* data, size_t n, int16_t* coef, size_t capacity_elems, pa_jpeg_desc* desc) {
    if (!data || !desc || !coef) return fail(1, "pa_jpeg_entropy_host: NULL argument");
    Header hd;
    int rc = parse_header(data, n, hd, true);
    if (rc) { memset(desc, 0, sizeof *desc); return rc; }
    rc = describe(hd, desc);
    if (rc) return rc;
    if ((uint64_t)desc->total_elems > (uint64_t)capacity_elems) {
        char msg[160];
        snprintf(msg, sizeof msg, "pa_jpeg_entropy_host: %lld coefficients do not fit a buffer of %zu", (long long)desc->total_elems, capacity_elems);
        return fail(PA_JPEG_CAPACITY, msg);
    }
    return entropy_decode(data, n, hd, *desc, coef);
}

// ------------------------------------------------------------------------------------------------ device
namespace {

// what the kernels derive from a descriptor: everything from (width, height, ncomp, h0, v0), nothing from the stored grids / offsets,
// so that no descriptor whose image fits Hs x Ws can send them outside the workspace or the frames
struct JpegGeom {
    int ok;                 // 0: leave the frame zero and sizes alone
    int w, h, ncomp, hs, vs;
    int bw[3], bh[3];
    int nblk[3];            // blocks per component
};

__device__ __forceinline__ JpegGeom jpeg_geom(const pa_jpeg_desc& d, int64_t base, int Hs, int Ws) {
    JpegGeom g;
    g.w = d.width; g.h = d.height; g.ncomp = d.ncomp;
    g.hs = d.comp[0].h; g.vs = d.comp[0].v;
    bool ok = (g.ncomp == 1 || g.ncomp == 3) && g.w >= 1 && g.h >= 1 && g.w <= Ws && g.h <= Hs && base >= 0 && (base & 7) == 0;
    if (g.ncomp == 1) { ok = ok && g.hs == 1 && g.vs == 1; }
    else ok = ok && ((g.hs == 1 && g.vs == 1) || (g.hs == 2 && g.vs == 1) || (g.hs == 2 && g.vs == 2)) &&
              d.comp[1].h == 1 && d.comp[1].v == 1 && d.comp[2].h == 1 && d.comp[2].v == 1;
    g.ok = ok ? 1 : 0;
    if (!ok) { g.hs = g.vs = 1; g.w = g.h = 1; g.ncomp = 0; }
    int mw = (g.w + 8 * g.hs - 1) / (8 * g.hs), mh = (g.h + 8 * g.vs - 1) / (8 * g.vs);
    for (int c = 0; c < 3; ++c) {
        int ch = c == 0 ? g.hs : 1, cv = c == 0 ? g.vs : 1;
        g.bw[c] = c < g.ncomp ? mw * ch : 0;
        g.bh[c] = c < g.ncomp ? mh * cv : 0;
        g.nblk[c] = g.bw[c] * g.bh[c];
    }
    return g;
}

// bytes of one component plane slot: the MCU-padded luma grid of the largest image (16-pixel MCUs at most)
__host__ __device__ __forceinline__ size_t jpeg_plane_bytes(int Hs, int Ws) {
    return (size_t)((Ws + 15) / 16 * 16) * (size_t)((Hs + 15) / 16 * 16);
}

#define JFIX(x) ((int)((x) * 8192 + 0.5))

// libjpeg's jidctint 1-D pass on eight values (in place), descaled by `shift`
__device__ __forceinline__ void idct8(int (&x)[8], int shift) {
    int z1 = (x[2] + x[6]) * JFIX(0.541196100);
    int tmp2 = z1 - x[6] * JFIX(1.847759065);
    int tmp3 = z1 + x[2] * JFIX(0.765366865);
    int tmp0 = (int)((unsigned)(x[0] + x[4]) << 13);
    int tmp1 = (int)((unsigned)(x[0] - x[4]) << 13);
    int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    int z5 = (z3 + z4) * JFIX(1.175875602);
    t0 *= JFIX(0.298631336);
    t1 *= JFIX(2.053119869);
    t2 *= JFIX(3.072711026);
    t3 *= JFIX(1.501321110);
    z1 *= -JFIX(0.899976223);
    z2 *= -JFIX(2.562915447);
    z3 = z3 * (-JFIX(1.961570560)) + z5;
    z4 = z4 * (-JFIX(0.390180644)) + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    const int r = 1 << (shift - 1);
    x[0] = (tmp10 + t3 + r) >> shift;
    x[7] = (tmp10 - t3 + r) >> shift;
    x[1] = (tmp11 + t2 + r) >> shift;
    x[6] = (tmp11 - t2 + r) >> shift;
    x[2] = (tmp12 + t1 + r) >> shift;
    x[5] = (tmp12 - t1 + r) >> shift;
    x[3] = (tmp13 + t0 + r) >> shift;
    x[4] = (tmp13 - t0 + r) >> shift;
}

// libjpeg's range_limit table (jdmaster.c prepare_range_limit_table) as arithmetic
__device__ __forceinline__ unsigned range_limit(int v) {
    int i = v & 1023;
    return i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896;
}

typedef short short8 __attribute__((ext_vector_type(8)));
typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));
typedef int int4v __attribute__((ext_vector_type(4)));
typedef unsigned uint2v __attribute__((ext_vector_type(2)));

constexpr int IDCT_THREADS = 256;                    // 8 lanes per block: 32 blocks per workgroup
constexpr int IDCT_BLOCKS = IDCT_THREADS / 8;
constexpr int IDCT_LDS_STRIDE = 72;                  // words per block: 64 + 8, so that the 8 blocks of a wave hit different banks

// (a) grid (ceil(max blocks per image / 32), B).  Lane j of a block: loads row j (16 bytes of coefficients, 16 of the quantisation
// table), dequantises into LDS; transforms column j; transforms row j, range-limits and stores its 8 bytes.
__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const pa_jpeg_desc* __restrict__ descs,
                                                                 const int64_t* __restrict__ coef_base, int Hs, int Ws, uint8_t* __restrict__ planes) {
    __shared__ int lds[IDCT_BLOCKS * IDCT_LDS_STRIDE];
    const int b = blockIdx.y;
    const pa_jpeg_desc& d = descs[b];
    const JpegGeom g = jpeg_geom(d, coef_base[b], Hs, Ws);
    const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
    int blk = blockIdx.x * IDCT_BLOCKS + lb;
    const int total = g.nblk[0] + g.nblk[1] + g.nblk[2];
    if (blockIdx.x * IDCT_BLOCKS >= total) return;   // the whole workgroup (uniform)
    const bool valid = blk < total;
    int c = 0;
    int64_t coff = 0;
    if (valid) {
        if (blk >= g.nblk[0]) { blk -= g.nblk[0]; coff += (int64_t)g.nblk[0] * 64; c = 1; }
        if (c == 1 && blk >= g.nblk[1]) { blk -= g.nblk[1]; coff += (int64_t)g.nblk[1] * 64; c = 2; }
    }
    int* w = lds + lb * IDCT_LDS_STRIDE;
    if (valid) {
        const short8 cv = *reinterpret_cast<const short8*>(coef + coef_base[b] + coff + (int64_t)blk * 64 + j * 8);
        const ushort8 qv = *reinterpret_cast<const ushort8*>(&d.quant[c][j * 8]);
        int4v lo, hi;
#pragma unroll
        for (int k = 0; k < 4; ++k) { lo[k] = (int)cv[k] * (int)qv[k]; hi[k] = (int)cv[k + 4] * (int)qv[k + 4]; }
        *reinterpret_cast<int4v*>(w + j * 8) = lo;
        *reinterpret_cast<int4v*>(w + j * 8 + 4) = hi;
    }
    __syncthreads();
    int x[8];
    if (valid) {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = w[k * 8 + j];
        idct8(x, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k * 8 + j] = x[k];
    }
    __syncthreads();
    if (valid) {
        const int4v lo = *reinterpret_cast<const int4v*>(w + j * 8), hi = *reinterpret_cast<const int4v*>(w + j * 8 + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { x[k] = lo[k]; x[k + 4] = hi[k]; }
        idct8(x, 18);
        uint2v o;
        o[0] = range_limit(x[0]) | (range_limit(x[1]) << 8) | (range_limit(x[2]) << 16) | (range_limit(x[3]) << 24);
        o[1] = range_limit(x[4]) | (range_limit(x[5]) << 8) | (range_limit(x[6]) << 16) | (range_limit(x[7]) << 24);
        const int by = blk / g.bw[c], bx = blk - by * g.bw[c];
        const size_t P = jpeg_plane_bytes(Hs, Ws);
        uint8_t* plane = planes + ((size_t)b * 3 + c) * P;
        *reinterpret_cast<uint2v*>(plane + (size_t)(by * 8 + j) * (g.bw[c] * 8) + bx * 8) = o;
    }
}

// jdsample.c: the chroma sample for output pixel (x, y) from a plane of dw x dh samples with row pitch `pitch`
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ pl, int pitch, int dw, int dh, int hs, int vs, int x, int y) {
    if (hs == 1) return pl[(size_t)y * pitch + x];
    const int xc = x >> 1;
    if (vs == 1) {                                    // h2v1_fancy_upsample
        const uint8_t* r = pl + (size_t)y * pitch;
        const int p = r[xc];
        if (x & 1) return xc == dw - 1 ? p : (3 * p + r[xc + 1] + 2) >> 2;
        return xc == 0 ? p : (3 * p + r[xc - 1] + 1) >> 2;
    }
    const int yc = y >> 1;                            // h2v2_fancy_upsample: the nearer row weighs 3, the further 1
    int yn = (y & 1) ? yc + 1 : yc - 1;
    yn = yn < 0 ? 0 : yn > dh - 1 ? dh - 1 : yn;
    const uint8_t* r0 = pl + (size_t)yc * pitch;
    const uint8_t* r1 = pl + (size_t)yn * pitch;
    const int cs = 3 * r0[xc] + r1[xc];
    if (x & 1) return xc == dw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * r0[xc + 1] + r1[xc + 1] + 7) >> 4;
    return xc == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * r0[xc - 1] + r1[xc - 1] + 8) >> 4;
}

#define JFX(x) ((int)((x) * 65536 + 0.5))
__device__ __forceinline__ unsigned clamp255(int v) { return v < 0 ? 0u : v > 255 ? 255u : (unsigned)v; }

constexpr int COLOR_THREADS = 128;
constexpr int COLOR_PX = 4;                           // pixels per thread: 12 bytes of a frame row

// (b) grid (ceil(ceil(Ws / 4) / 128), Hs, B): a thread writes pixels x0 .. x0 + 3 of row y of frame b -- the image inside (w, h), zero outside
__global__ __launch_bounds__(COLOR_THREADS) void jpeg_color_kernel(const pa_jpeg_desc* __restrict__ descs, const int64_t* __restrict__ coef_base, int Hs, int Ws,
                                                                   const uint8_t* __restrict__ planes, uint8_t* __restrict__ frames,
                                                                   int32_t* __restrict__ sizes) {
    const int b = blockIdx.z, y = blockIdx.y;
    const int x0 = (blockIdx.x * COLOR_THREADS + threadIdx.x) * COLOR_PX;
    if (x0 >= Ws) return;
    const JpegGeom g = jpeg_geom(descs[b], coef_base[b], Hs, Ws);
    if (g.ok && y == 0 && x0 == 0) { sizes[2 * b] = g.w; sizes[2 * b + 1] = g.h; }
    unsigned px[COLOR_PX][3];
#pragma unroll
    for (int i = 0; i < COLOR_PX; ++i) px[i][0] = px[i][1] = px[i][2] = 0;
    if (g.ok && y < g.h && x0 < g.w) {
        const size_t P = jpeg_plane_bytes(Hs, Ws);
        const uint8_t* p0 = planes + (size_t)b * 3 * P;
        const int pitch0 = g.bw[0] * 8;
        const unsigned yy = *reinterpret_cast<const unsigned*>(p0 + (size_t)y * pitch0 + x0);     // x0 % 4 == 0, pitch0 % 8 == 0, x0 + 3 < pitch0
        if (g.ncomp == 1) {
#pragma unroll
            for (int i = 0; i < COLOR_PX; ++i) px[i][0] = px[i][1] = px[i][2] = x0 + i < g.w ? (yy >> (8 * i)) & 255 : 0u;
        } else {
            const int pitch1 = g.bw[1] * 8;
            const int dw = (g.w + g.hs - 1) / g.hs, dh = (g.h + g.vs - 1) / g.vs;
            const uint8_t* p1 = p0 + P;
            const uint8_t* p2 = p0 + 2 * P;
#pragma unroll
            for (int i = 0; i < COLOR_PX; ++i) {
                const int x = x0 + i;
                if (x < g.w) {
                    const int Y = (yy >> (8 * i)) & 255;
                    const int cb = chroma_at(p1, pitch1, dw, dh, g.hs, g.vs, x, y) - 128;
                    const int cr = chroma_at(p2, pitch1, dw, dh, g.hs, g.vs, x, y) - 128;
                    px[i][0] = clamp255(Y + ((JFX(1.40200) * cr + 32768) >> 16));
                    px[i][1] = clamp255(Y + ((-JFX(0.34414) * cb + 32768 - JFX(0.71414) * cr) >> 16));
                    px[i][2] = clamp255(Y + ((JFX(1.77200) * cb + 32768) >> 16));
                }
            }
        }
    }
    uint8_t* out = frames + (((size_t)b * Hs + y) * Ws + x0) * 3;
    if (x0 + COLOR_PX <= Ws && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        unsigned* o = reinterpret_cast<unsigned*>(out);
        o[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
        o[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
        o[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < COLOR_PX; ++i)
            if (x0 + i < Ws) {
                out[3 * i] = (uint8_t)px[i][0];
                out[3 * i + 1] = (uint8_t)px[i][1];
                out[3 * i + 2] = (uint8_t)px[i][2];
            }
    }
}

}  // namespace

extern "C" size_t pa_jpeg_workspace_bytes(int B, int Hs, int Ws) {
    if (B <= 0 || Hs <= 0 || Ws <= 0) return 0;
    return (size_t)B * 3 * jpeg_plane_bytes(Hs, Ws);
}

extern "C" int pa_jpeg_decode(const int16_t* coef, const pa_jpeg_desc* descs, const int64_t* coef_base, int B, int Hs, int Ws,
                              void* workspace, uint8_t* frames, int32_t* sizes, void* stream) {
    if (!coef || !descs || !coef_base || !workspace || !frames || !sizes || B <= 0 || Hs <= 0 || Ws <= 0 || B > 65535 || Hs > 65535 ||
        Ws > 65535) {
        pa_set_error_msg("pa_jpeg_decode: bad arguments (NULL pointer, or B / Hs / Ws outside 1 .. 65535)");
        return 1;
    }
    if ((reinterpret_cast<uintptr_t>(coef) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(descs) & 15)) {
        pa_set_error_msg("pa_jpeg_decode: coef, descs and workspace must be 16-byte aligned");
        return 1;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t max_blocks = 3 * jpeg_plane_bytes(Hs, Ws) / 64;
    dim3 ga((unsigned)((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), (unsigned)B);
    hipLaunchKernelGGL(jpeg_idct_kernel, ga, dim3(IDCT_THREADS), 0, s, coef, descs, coef_base, Hs, Ws, static_cast<uint8_t*>(workspace));
    PA_CHECK(hipGetLastError());
    const int tx = (Ws + COLOR_PX - 1) / COLOR_PX;
    dim3 gb((unsigned)((tx + COLOR_THREADS - 1) / COLOR_THREADS), (unsigned)Hs, (unsigned)B);
    hipLaunchKernelGGL(jpeg_color_kernel, gb, dim3(COLOR_THREADS), 0, s, descs, coef_base, Hs, Ws, static_cast<const uint8_t*>(workspace), frames, sizes);
    PA_CHECK(hipGetLastError());
    return 0;
}
