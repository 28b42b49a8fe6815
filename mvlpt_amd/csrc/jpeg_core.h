// Baseline JPEG decode, bit-exact with libjpeg(-turbo) as Pillow drives it: the arithmetic the kernels of jpeg.hip run, written as
// __host__ __device__ functions so that a CPU build (tools/jpeg_core_check.cpp, under the address and undefined-behaviour sanitizers)
// executes the same text, and the file parser, plain C++ for the host.
//   entropy   jdhuff.c: MSB-first bits, FF 00 = a stuffed FF, 8-bit lookahead + a bounded slow path to 16 bits, DC predictors reset per
//             restart segment.  A segment never reads outside [begin, end): past the end it is fed zero bytes, and having consumed one
//             of them is an error (ST_ENDED_EARLY)
//   IDCT      jidctint.c jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2), in uint32 so that overflow wraps and is defined
//   upsample  jdsample.c "fancy" h2v1 / h2v2 (triangle filter) over the component's down-sampled size; a component at most two
//             samples wide is replicated instead, as jinit_upsampler chooses
//   colour    jdcolor.c YCbCr -> RGB, 16-bit fixed point
#ifndef MVLPT_JPEG_CORE_H
#define MVLPT_JPEG_CORE_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif

namespace mvlpt {
namespace jpeg {

// MvlptJpegInfo.route: 0 = the device decodes it, anything else names why the host (Pillow) does
enum Route {
  ROUTE_DEVICE = 0,
  ROUTE_MALFORMED = 1,      // no SOI, a marker where none may stand, a marker length that runs past the file, no frame / scan header
  ROUTE_FRAME = 2,          // not SOF0 with 8-bit samples: progressive, arithmetic, extended, lossless, 12-bit
  ROUTE_SCANS = 3,          // more than one scan, a scan that does not interleave every component, DNL
  ROUTE_COLOUR = 4,         // not grayscale or JFIF YCbCr: CMYK / YCCK, Adobe APP14, RGB component ids
  ROUTE_SAMPLING = 5,       // luma not 1x1, 2x1 or 2x2, or chroma not 1x1
  ROUTE_TABLES = 6,         // a table the scan names is missing, 16-bit, outside baseline's ids, or not a prefix code
  ROUTE_RESTART = 7,        // RSTn out of sequence, or not ceil(MCUs / DRI) - 1 of them
  ROUTE_SIZE = 8            // an empty image, or one beyond the 2^26 pixels the 32-bit indices are sized for
};
// status word of an image the device decoded (a sum of these): > 0 = corrupt entropy data
enum Status { ST_BAD_CODE = 1, ST_COEF_INDEX = 2, ST_ENDED_EARLY = 4, ST_BAD_SIZE = 8 };

constexpr int64_t MAX_PIXELS = (int64_t)1 << 26;

// one image's tables as they are uploaded: quantisation in natural (de-zigzagged) order, Huffman as DHT holds them.
// Huffman slot = class * 2 + id (DC 0, DC 1, AC 0, AC 1)
struct Tables {
  uint8_t q[4][64];
  uint8_t bits[4][17];       // bits[t][l] codes of length l, l = 1 .. 16
  uint8_t pad[4];
  uint8_t vals[4][256];
};
static_assert(sizeof(Tables) == 1352, "Tables is uploaded as bytes");

// the decoder's view of the four Huffman tables (LDS on the device)
struct HuffLut {
  uint16_t look[4][256];     // next 8 bits -> (length << 8) | symbol, 0 when the code is longer
  int32_t maxcode[4][18];    // largest code of length l, -1 when there is none
  int32_t valoff[4][17];     // index of the first symbol of length l, minus its code
  uint8_t vals[4][256];
};

struct Seg { uint32_t begin, end; };   // entropy bytes [begin, end) of one restart segment, offsets into the file

// what the kernels read about one image (uploaded with the call)
struct ImgDesc {
  int64_t src_off;           // the file's first byte in the compressed source
  int64_t dst_off;           // byte offset of pixel (0, 0) in the packed HWC RGB destination
  int64_t coef_off[3];       // first coefficient block of each component in the workspace
  int64_t plane_off[3];      // first byte of each component plane
  int32_t plane_w[3];        // plane pitch = blocks per row * 8 (whole MCUs)
  int32_t plane_h[3];
  int32_t blocks_w[3];
  int32_t seg_first, n_segs; // rows of the segment table
  int32_t restart;           // MCUs per segment
  int32_t width, height, ncomp, hs, vs, mcux, mcuy;
  int32_t tables;            // row of the table sets
  int32_t tq[3], td[3], ta[3];
  int32_t index;             // row of the status array
  int32_t reserved;
};

// one component of one image, as the IDCT kernel sees it
struct PlaneDesc {
  int64_t coef_off, plane_off;
  int32_t n_blocks, blocks_w, plane_w;
  int32_t tables, tq, reserved;
};

JPEG_HD int zigzag(int k) {
  static const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return zz[k & 63];
}

// ------------------------------------------------------------------------------------------------ Huffman tables
// jpeg_make_d_derived_tbl for table t.  Every loop has a constant bound and every index is masked, whatever `bits` holds.
JPEG_HD void build_lut(const Tables& T, int t, HuffLut& L) {
  for (int i = 0; i < 256; ++i) { L.look[t][i] = 0; L.vals[t][i] = T.vals[t][i]; }
  int p = 0, code = 0;
  L.maxcode[t][0] = -1;
  L.valoff[t][0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = T.bits[t][l];
    L.valoff[t][l] = p - code;
    L.maxcode[t][l] = n ? code + n - 1 : -1;
    if (l <= 8) {
      for (int i = 0; i < n; ++i) {
        const int c = (code + i) << (8 - l);
        for (int k = 0; k < (1 << (8 - l)); ++k) L.look[t][(c + k) & 255] = (uint16_t)((l << 8) | T.vals[t][(p + i) & 255]);
      }
    }
    p += n;
    code = (code + n) << 1;
  }
  L.maxcode[t][17] = 0xFFFFF;
}

// ------------------------------------------------------------------------------------------------ entropy decode
struct BitReader {
  const uint8_t* p;
  uint32_t pos, end;
  uint64_t buf;             // the low n bits are the next n bits of the stream
  int n;
  uint32_t zeros;           // zero bytes fed past the end
};

// at least 57 bits afterwards
JPEG_HD void br_fill(BitReader& r) {
  for (int it = 0; it < 8 && r.n <= 56; ++it) {
    if (r.n <= 32 && r.pos + 4 <= r.end) {                       // four bytes at once when none is FF
      const uint32_t b0 = r.p[r.pos], b1 = r.p[r.pos + 1], b2 = r.p[r.pos + 2], b3 = r.p[r.pos + 3];
      if (b0 != 0xFF && b1 != 0xFF && b2 != 0xFF && b3 != 0xFF) {
        r.buf = (r.buf << 32) | (uint64_t)((b0 << 24) | (b1 << 16) | (b2 << 8) | b3);
        r.n += 32;
        r.pos += 4;
        continue;
      }
    }
    uint32_t b = 0;
    if (r.pos < r.end) {
      b = r.p[r.pos++];
      if (b == 0xFF) {
        if (r.pos < r.end && r.p[r.pos] == 0) ++r.pos;           // stuffed
        else { r.pos = r.end; b = 0; ++r.zeros; }                // a marker, or the file's last byte: the data stops here
      }
    } else {
      ++r.zeros;
    }
    r.buf = (r.buf << 8) | b;
    r.n += 8;
  }
}
JPEG_HD int br_get(BitReader& r, int l) {                        // 1 <= l <= 16 <= r.n
  r.n -= l;
  return (int)((r.buf >> r.n) & ((1u << l) - 1u));
}
// symbol of table t, or -1 when the next 16 bits match no code
JPEG_HD int huff_decode(BitReader& r, const HuffLut& L, int t) {
  const int e = L.look[t][(r.buf >> (r.n - 8)) & 255];
  if (e) { r.n -= e >> 8; return e & 255; }
  for (int l = 9; l <= 16; ++l) {
    const int c = (int)((r.buf >> (r.n - l)) & ((1u << l) - 1u));
    if (c <= L.maxcode[t][l]) { r.n -= l; return L.vals[t][(c + L.valoff[t][l]) & 255]; }
  }
  return -1;
}
JPEG_HD int extend(int v, int s) { return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1; }

// MCUs [mcu_first, mcu_first + mcu_count) of image d from the bytes [begin, end) of `file`, into the (zeroed) coefficient blocks
// coefs[coef_off[c] ..] (int16 [64], natural order).  Returns the Status bits; on an error the segment stops.
JPEG_HD int decode_segment(const uint8_t* file, uint32_t begin, uint32_t end, const ImgDesc& d, const HuffLut& L, int mcu_first,
                           int mcu_count, int16_t* coefs) {
  BitReader r = {file, begin, end < begin ? begin : end, 0, 0, 0};
  int pred[3] = {0, 0, 0};
  int my = mcu_first / d.mcux, mx = mcu_first - my * d.mcux;
  for (int m = 0; m < mcu_count; ++m) {
    for (int c = 0; c < d.ncomp; ++c) {
      const int hb = c == 0 ? d.hs : 1, vb = c == 0 ? d.vs : 1;
      for (int by = 0; by < vb; ++by) {
        for (int bx = 0; bx < hb; ++bx) {
          int16_t* blk = coefs + (d.coef_off[c] + (int64_t)(my * vb + by) * d.blocks_w[c] + mx * hb + bx) * 64;
          br_fill(r);
          int s = huff_decode(r, L, d.td[c]);
          if (s < 0) return ST_BAD_CODE;
          if (s > 15) return ST_BAD_SIZE;
          if (s) pred[c] = (int)((uint32_t)pred[c] + (uint32_t)extend(br_get(r, s), s));
          if (pred[c]) blk[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            br_fill(r);
            const int rs = huff_decode(r, L, 2 + d.ta[c]);
            if (rs < 0) return ST_BAD_CODE;
            const int run = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (run != 15) break;                              // EOB
              k += 16;                                           // ZRL
              continue;
            }
            k += run;
            if (k > 63) return ST_COEF_INDEX;
            blk[zigzag(k)] = (int16_t)extend(br_get(r, s), s);
            ++k;
          }
        }
      }
    }
    if (++mx == d.mcux) { mx = 0; ++my; }
  }
  return (int64_t)r.zeros * 8 > r.n ? ST_ENDED_EARLY : 0;
}

// ------------------------------------------------------------------------------------------------ IDCT
// One pass of jpeg_idct_islow over eight values: out = DESCALE(..., shift).  uint32 arithmetic, arithmetic right shift.
JPEG_HD void idct_1d(const int32_t* in, int32_t* out, int shift) {
  typedef uint32_t u;
  const u rnd = (u)1 << (shift - 1);
  u z2 = (u)in[2], z3 = (u)in[6];
  u z1 = (z2 + z3) * 4433u;
  u tmp2 = z1 - z3 * 15137u;
  u tmp3 = z1 + z2 * 6270u;
  z2 = (u)in[0]; z3 = (u)in[4];
  u tmp0 = (z2 + z3) << 13;
  u tmp1 = (z2 - z3) << 13;
  const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = (u)in[7]; tmp1 = (u)in[5]; tmp2 = (u)in[3]; tmp3 = (u)in[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  u z4 = tmp1 + tmp3;
  const u z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
  z1 *= (u)-7373; z2 *= (u)-20995; z3 *= (u)-16069; z4 *= (u)-3196;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  out[0] = (int32_t)(tmp10 + tmp3 + rnd) >> shift;
  out[7] = (int32_t)(tmp10 - tmp3 + rnd) >> shift;
  out[1] = (int32_t)(tmp11 + tmp2 + rnd) >> shift;
  out[6] = (int32_t)(tmp11 - tmp2 + rnd) >> shift;
  out[2] = (int32_t)(tmp12 + tmp1 + rnd) >> shift;
  out[5] = (int32_t)(tmp12 - tmp1 + rnd) >> shift;
  out[3] = (int32_t)(tmp13 + tmp0 + rnd) >> shift;
  out[4] = (int32_t)(tmp13 - tmp0 + rnd) >> shift;
}
JPEG_HD uint8_t clamp8(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
// column x of a block: dequantise, pass 1 into ws[8 * k + x]
JPEG_HD void idct_column(const int16_t* coef, const uint8_t* q, int x, int32_t* ws) {
  int32_t in[8], out[8];
  for (int k = 0; k < 8; ++k) in[k] = (int32_t)coef[8 * k + x] * (int32_t)q[8 * k + x];
  idct_1d(in, out, 11);
  for (int k = 0; k < 8; ++k) ws[8 * k + x] = out[k];
}
// row y of a block: pass 2 over ws[8 * y ..], + 128, clamp
JPEG_HD void idct_row(const int32_t* ws, int y, uint8_t* px) {
  int32_t out[8];
  idct_1d(ws + 8 * y, out, 18);
  for (int k = 0; k < 8; ++k) px[k] = clamp8(out[k] + 128);
}

// ------------------------------------------------------------------------------------------------ upsample + colour
// chroma sample at luma position (y, x): pl is the component plane (pitch `stride`), cw x ch its down-sampled size
JPEG_HD int chroma_at(const uint8_t* pl, int stride, int cw, int ch, int hs, int vs, int y, int x) {
  if (hs == 1) return pl[(size_t)y * stride + x];
  if (cw <= 2) return pl[(size_t)(vs == 2 ? y >> 1 : y) * stride + (x >> 1)];     // replicated (jinit_upsampler: downsampled_width <= 2)
  const int i = x >> 1;
  if (vs == 1) {
    const uint8_t* row = pl + (size_t)y * stride;
    const int c = row[i];
    if (x == 0 || x == 2 * cw - 1) return c;
    return (x & 1) ? (3 * c + row[i + 1] + 2) >> 2 : (3 * c + row[i - 1] + 1) >> 2;
  }
  const int j = y >> 1;
  int f = (y & 1) ? j + 1 : j - 1;
  f = f < 0 ? 0 : (f > ch - 1 ? ch - 1 : f);
  const uint8_t* near = pl + (size_t)j * stride;
  const uint8_t* far = pl + (size_t)f * stride;
  const int t = 3 * near[i] + far[i];
  if (x == 0) return (4 * t + 8) >> 4;
  if (x == 2 * cw - 1) return (4 * t + 7) >> 4;
  return (x & 1) ? (3 * t + 3 * near[i + 1] + far[i + 1] + 7) >> 4 : (3 * t + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}
JPEG_HD void ycc_to_rgb(int y, int cb, int cr, uint8_t* rgb) {
  cb -= 128; cr -= 128;
  rgb[0] = clamp8(y + ((91881 * cr + 32768) >> 16));
  rgb[1] = clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = clamp8(y + ((116130 * cb + 32768) >> 16));
}
// pixel (y, x) of image d from its component planes
JPEG_HD void pixel_rgb(const ImgDesc& d, const uint8_t* planes, int y, int x, uint8_t* rgb) {
  const int Y = planes[d.plane_off[0] + (int64_t)y * d.plane_w[0] + x];
  if (d.ncomp == 1) { rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y; return; }
  const int cw = (d.width + d.hs - 1) / d.hs, ch = (d.height + d.vs - 1) / d.vs;
  const int cb = chroma_at(planes + d.plane_off[1], d.plane_w[1], cw, ch, d.hs, d.vs, y, x);
  const int cr = chroma_at(planes + d.plane_off[2], d.plane_w[2], cw, ch, d.hs, d.vs, y, x);
  ycc_to_rgb(Y, cb, cr, rgb);
}

// ------------------------------------------------------------------------------------------------ host: geometry and parser
struct Info {                // = MvlptJpegInfo
  int32_t height, width, components, h_samp, v_samp, restart_interval, n_segments, route;
};
struct Geom {
  int mcux, mcuy;
  int64_t blocks[3], plane_bytes[3];
  int blocks_w[3], plane_w[3], plane_h[3];
  int64_t total_blocks, total_plane_bytes;
};
// a grayscale scan is not interleaved: its MCU is one block whatever sampling factors the frame names
inline Geom geometry(const Info& f) {
  Geom g = {};
  const int hs = f.components == 1 ? 1 : f.h_samp, vs = f.components == 1 ? 1 : f.v_samp;
  g.mcux = (f.width + 8 * hs - 1) / (8 * hs);
  g.mcuy = (f.height + 8 * vs - 1) / (8 * vs);
  for (int c = 0; c < f.components && c < 3; ++c) {
    const int hb = c == 0 ? hs : 1, vb = c == 0 ? vs : 1;
    g.blocks_w[c] = g.mcux * hb;
    g.plane_w[c] = g.blocks_w[c] * 8;
    g.plane_h[c] = g.mcuy * vb * 8;
    g.blocks[c] = (int64_t)g.blocks_w[c] * g.mcuy * vb;
    g.plane_bytes[c] = g.blocks[c] * 64;
    g.total_blocks += g.blocks[c];
    g.total_plane_bytes += g.plane_bytes[c];
  }
  return g;
}

struct Parsed {
  Info info;
  Tables tables;
  int tq[3], td[3], ta[3];
  std::vector<Seg> segs;
};

// Reads the headers and delimits the restart segments.  Never reads outside [0, n).  info.route says who decodes the file; the other
// fields of info hold whatever the headers gave before the verdict (0 when the frame header was not reached).
inline void parse(const uint8_t* p, size_t n, Parsed* out) {
  Parsed& P = *out;
  memset(&P.info, 0, sizeof(P.info));
  memset(&P.tables, 0, sizeof(P.tables));
  for (int c = 0; c < 3; ++c) P.tq[c] = P.td[c] = P.ta[c] = 0;
  P.segs.clear();
  Info& I = P.info;
  auto verdict = [&](int route) { I.route = route; };
  if (n < 4 || n >= ((size_t)1 << 31) || p[0] != 0xFF || p[1] != 0xD8) return verdict(ROUTE_MALFORMED);
  size_t pos = 2;
  bool jfif = false, adobe = false, bad_tables = false, have_sof = false;
  int sof = 0, precision = 0, nf = 0, dri = 0;
  unsigned q_defined = 0, q_wide = 0, h_defined = 0;
  int comp_id[4] = {0, 0, 0, 0}, comp_h[4] = {0, 0, 0, 0}, comp_v[4] = {0, 0, 0, 0}, comp_tq[4] = {0, 0, 0, 0};
  size_t scan = 0;                                               // first entropy byte
  int ns = 0, scan_id[4] = {0, 0, 0, 0}, scan_t[4] = {0, 0, 0, 0}, ss = 0, se = 0, ahal = 0;
  for (;;) {
    if (pos + 2 > n) return verdict(ROUTE_MALFORMED);
    if (p[pos] != 0xFF) return verdict(ROUTE_MALFORMED);
    while (pos < n && p[pos] == 0xFF) ++pos;
    if (pos >= n) return verdict(ROUTE_MALFORMED);
    const int m = p[pos++];
    if (m == 0 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return verdict(ROUTE_MALFORMED);   // stand-alone markers have no place here
    if (pos + 2 > n) return verdict(ROUTE_MALFORMED);
    const size_t len = ((size_t)p[pos] << 8) | p[pos + 1];
    if (len < 2 || pos + len > n) return verdict(ROUTE_MALFORMED);
    const uint8_t* s = p + pos + 2;
    size_t sl = len - 2;
    if (m == 0xE0) {
      if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) adobe = true;
    } else if (m == 0xDB) {
      while (sl > 0) {
        const int pq = s[0] >> 4, t = s[0] & 15;
        const size_t need = 1 + (pq ? 128 : 64);
        if (pq > 1 || t > 3 || sl < need) return verdict(ROUTE_MALFORMED);
        if (pq == 0) {
          for (int k = 0; k < 64; ++k) P.tables.q[t][zigzag(k)] = s[1 + k];
          q_wide &= ~(1u << t);
        } else {
          q_wide |= 1u << t;
        }
        q_defined |= 1u << t;
        s += need; sl -= need;
      }
    } else if (m == 0xC4) {
      while (sl > 0) {
        if (sl < 17) return verdict(ROUTE_MALFORMED);
        const int tc = s[0] >> 4, th = s[0] & 15;
        if (tc > 1 || th > 3) return verdict(ROUTE_MALFORMED);
        size_t count = 0;
        for (int l = 1; l <= 16; ++l) count += s[l];
        if (count > 256 || sl < 17 + count) return verdict(ROUTE_MALFORMED);
        if (th < 2) {
          const int t = tc * 2 + th;
          bool ok = true;
          int code = 0;
          P.tables.bits[t][0] = 0;
          for (int l = 1; l <= 16; ++l) {                        // a prefix code: no length has more codes than are left
            P.tables.bits[t][l] = s[l];
            code += s[l];
            if (code > (1 << l)) ok = false;
            code <<= 1;
          }
          memset(P.tables.vals[t], 0, 256);
          for (size_t k = 0; k < count; ++k) {
            P.tables.vals[t][k] = s[17 + k];
            if (tc == 0 && s[17 + k] > 15) ok = false;           // a DC symbol is a bit count
          }
          if (ok) h_defined |= 1u << t; else { h_defined &= ~(1u << t); bad_tables = true; }
        }
        s += 17 + count; sl -= 17 + count;
      }
    } else if (m == 0xDD) {
      if (sl < 2) return verdict(ROUTE_MALFORMED);
      dri = (s[0] << 8) | s[1];
    } else if (m == 0xDC) {
      return verdict(ROUTE_SCANS);
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {   // a frame header (C4 and DD were taken above)
      if (have_sof || sl < 6) return verdict(ROUTE_MALFORMED);
      have_sof = true;
      sof = m;
      precision = s[0];
      I.height = (s[1] << 8) | s[2];
      I.width = (s[3] << 8) | s[4];
      nf = s[5];
      I.components = nf;
      if (sl < 6 + 3 * (size_t)nf) return verdict(ROUTE_MALFORMED);
      for (int c = 0; c < nf && c < 4; ++c) {
        comp_id[c] = s[6 + 3 * c];
        comp_h[c] = s[7 + 3 * c] >> 4;
        comp_v[c] = s[7 + 3 * c] & 15;
        comp_tq[c] = s[8 + 3 * c];
      }
      I.h_samp = comp_h[0];
      I.v_samp = comp_v[0];
    } else if (m == 0xDA) {
      if (!have_sof || sl < 1) return verdict(ROUTE_MALFORMED);
      ns = s[0];
      if (ns < 1 || ns > 4 || sl < 4 + 2 * (size_t)ns) return verdict(ROUTE_MALFORMED);
      for (int c = 0; c < ns; ++c) { scan_id[c] = s[1 + 2 * c]; scan_t[c] = s[2 + 2 * c]; }
      ss = s[1 + 2 * ns]; se = s[2 + 2 * ns]; ahal = s[3 + 2 * ns];
      scan = pos + len;
      break;
    }
    pos += len;
  }
  I.restart_interval = dri;
  if (sof != 0xC0 || precision != 8) return verdict(ROUTE_FRAME);
  if (I.height <= 0 || I.width <= 0 || (int64_t)I.height * I.width > MAX_PIXELS) return verdict(ROUTE_SIZE);
  if (nf != 1 && nf != 3) return verdict(ROUTE_COLOUR);
  if (nf == 3) {
    if (adobe) return verdict(ROUTE_COLOUR);
    if (!jfif && !(comp_id[0] == 1 && comp_id[1] == 2 && comp_id[2] == 3)) return verdict(ROUTE_COLOUR);
    const bool luma_ok = (comp_h[0] == 1 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 2);
    if (!luma_ok || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) return verdict(ROUTE_SAMPLING);
  } else if (comp_h[0] < 1 || comp_h[0] > 4 || comp_v[0] < 1 || comp_v[0] > 4) {
    return verdict(ROUTE_MALFORMED);
  }
  if (ns != nf || ss != 0 || se != 63 || ahal != 0) return verdict(ROUTE_SCANS);
  for (int c = 0; c < nf; ++c) {
    if (scan_id[c] != comp_id[c]) return verdict(ROUTE_SCANS);
    const int td = scan_t[c] >> 4, ta = scan_t[c] & 15, tq = comp_tq[c];
    if (td > 1 || ta > 1 || tq > 3 || bad_tables) return verdict(ROUTE_TABLES);
    if (!(h_defined >> td & 1u) || !(h_defined >> (2 + ta) & 1u) || !(q_defined >> tq & 1u) || (q_wide >> tq & 1u)) return verdict(ROUTE_TABLES);
    P.tq[c] = tq; P.td[c] = td; P.ta[c] = ta;
  }
  // the entropy data: restart segments up to EOI (or to the end of a file that was cut)
  size_t i = scan, seg_begin = scan;
  int expected = 0;
  bool closed = false;
  while (i < n) {
    if (p[i] != 0xFF) { ++i; continue; }
    size_t j = i;
    while (j < n && p[j] == 0xFF) ++j;
    if (j >= n) break;                                           // the file ends in FF: the reader stops there
    const int m = p[j];
    if (m == 0) {
      if (j - i != 1) return verdict(ROUTE_RESTART);             // fill bytes inside the entropy data
      i = j + 1;
      continue;
    }
    if (m >= 0xD0 && m <= 0xD7) {
      if (m - 0xD0 != (expected & 7)) return verdict(ROUTE_RESTART);
      ++expected;
      P.segs.push_back(Seg{(uint32_t)seg_begin, (uint32_t)i});
      seg_begin = i = j + 1;
      continue;
    }
    if (m != 0xD9) return verdict(ROUTE_SCANS);                  // tables or another scan behind this one
    P.segs.push_back(Seg{(uint32_t)seg_begin, (uint32_t)i});
    closed = true;
    break;
  }
  if (!closed) P.segs.push_back(Seg{(uint32_t)seg_begin, (uint32_t)n});
  I.n_segments = (int32_t)P.segs.size();
  const Geom g = geometry(I);
  const int64_t mcus = (int64_t)g.mcux * g.mcuy;
  const int64_t want = dri > 0 ? (mcus + dri - 1) / dri : 1;
  if ((int64_t)P.segs.size() != want) return verdict(ROUTE_RESTART);
  return verdict(ROUTE_DEVICE);
}

// the descriptor of a device-route image; coefficient blocks from block `coef_base`, planes from byte `plane_base`
inline ImgDesc describe(const Parsed& P, int64_t src_off, int64_t dst_off, int64_t coef_base, int64_t plane_base, int seg_first,
                        int tables, int index) {
  const Info& I = P.info;
  const Geom g = geometry(I);
  ImgDesc d;
  memset(&d, 0, sizeof(d));
  d.src_off = src_off; d.dst_off = dst_off;
  for (int c = 0; c < I.components; ++c) {
    d.coef_off[c] = coef_base; coef_base += g.blocks[c];
    d.plane_off[c] = plane_base; plane_base += g.plane_bytes[c];
    d.plane_w[c] = g.plane_w[c]; d.plane_h[c] = g.plane_h[c]; d.blocks_w[c] = g.blocks_w[c];
    d.tq[c] = P.tq[c]; d.td[c] = P.td[c]; d.ta[c] = P.ta[c];
  }
  d.seg_first = seg_first; d.n_segs = I.n_segments;
  d.restart = I.restart_interval > 0 ? I.restart_interval : g.mcux * g.mcuy;
  d.width = I.width; d.height = I.height; d.ncomp = I.components;
  d.hs = I.components == 1 ? 1 : I.h_samp; d.vs = I.components == 1 ? 1 : I.v_samp;
  d.mcux = g.mcux; d.mcuy = g.mcuy;
  d.tables = tables; d.index = index;
  return d;
}

}  // namespace jpeg
}  // namespace mvlpt
#endif  // MVLPT_JPEG_CORE_H
