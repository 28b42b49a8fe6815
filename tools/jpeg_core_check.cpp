// CPU run of mvlpt_amd/csrc/jpeg_core.h, the text the kernels of jpeg.hip execute, meant for
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mvlpt_amd/csrc tools/jpeg_core_check.cpp
// (tests/test_jpeg_core_sanitized.py builds and runs it).  Every buffer is a heap block of exactly the size the C ABI computes
// (mvlpt_jpeg_workspace_bytes' terms: coefficient blocks, component planes; H * W * 3 destination bytes; the file itself), so a read or
// write one byte outside any of them is a sanitizer report.
//
//   jpeg_core_check CASES [MUTATIONS_PER_FILE] [SEED]
// CASES (written by the test from tests/golden/jpeg.npz): u32 count, then per case u32 kind (0 supported, 1 fallback, 2 malformed),
// u32 jpeg bytes, u32 pixel bytes (0: Pillow cannot read the file), the JPEG, the RGB pixels Pillow decoded.
//   kind 0: route device, status 0, pixels equal.   kind 1: a fallback route.   kind 2: route device and a status > 0.
//   kind 3 (a mutated or truncated file the test made, with the pixels Pillow decodes from it, none if Pillow cannot read it): a fallback
//   route, or a status > 0, or pixels equal to Pillow's -- or, counted apart, damaged values beyond the IDCT's number range (Result::in_range below).
// Then MUTATIONS_PER_FILE further seeded mutations of every kind-0 file, made here (a byte replaced in the headers, a byte replaced or a
// bit flipped in the entropy data, a truncation), go through the same path with no reference to compare with: a mutation can produce
// another VALID file (a changed quantisation value, a code swapped for one of equal length), so their outcome is tallied, and what is
// asserted for them is what the sanitizers assert: nothing was touched outside the buffers.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "jpeg_core.h"

using namespace mvlpt::jpeg;

// in_range: every dequantised coefficient and every output of the IDCT's first pass fits 16 bits -- the number format libjpeg-turbo's SIMD
// IDCT keeps them in -- and every output of the second pass lies in [-512, 511], the window of jidctint.c's range table.  Outside it
// libjpeg's own implementations (C: 32-bit and a range table that WRAPS; SIMD: saturating 16-bit) give different pixels, and the device's
// decode, which is the C arithmetic with a clamp, is promised equal to neither: no encoder writes such values.
struct Result { int route = 0, status = 0; bool in_range = true; std::vector<uint8_t> rgb; };

static Result decode(const uint8_t* bytes, size_t n) {
  Result R;
  std::unique_ptr<uint8_t[]> file(new uint8_t[n ? n : 1]);      // exact size: an over-read of the file is caught
  memcpy(file.get(), bytes, n);
  Parsed P;
  parse(file.get(), n, &P);
  R.route = P.info.route;
  if (R.route != ROUTE_DEVICE) return R;
  const Geom g = geometry(P.info);
  const ImgDesc d = describe(P, 0, 0, 0, 0, 0, 0, 0);
  std::unique_ptr<int16_t[]> coefs(new int16_t[g.total_blocks * 64]());
  std::unique_ptr<uint8_t[]> planes(new uint8_t[g.total_plane_bytes]());
  R.rgb.assign((size_t)d.width * d.height * 3, 0);
  std::unique_ptr<HuffLut> L(new HuffLut);
  for (int t = 0; t < 4; ++t) build_lut(P.tables, t, *L);
  const int mcus = d.mcux * d.mcuy;
  for (int s = 0; s < d.n_segs; ++s) {
    const int first = s * d.restart, count = mcus - first < d.restart ? mcus - first : d.restart;
    R.status |= decode_segment(file.get(), P.segs[s].begin, P.segs[s].end, d, *L, first, count, coefs.get());
  }
  for (int c = 0; c < d.ncomp; ++c) {
    const int64_t nb = g.blocks[c];
    for (int64_t b = 0; b < nb; ++b) {
      int32_t ws[64];
      const int16_t* blk = coefs.get() + (d.coef_off[c] + b) * 64;
      for (int x = 0; x < 8; ++x) idct_column(blk, P.tables.q[d.tq[c]], x, ws);
      for (int k = 0; k < 64; ++k) {
        const int32_t dq = (int32_t)blk[k] * P.tables.q[d.tq[c]][k];
        if (dq < -32768 || dq > 32767 || ws[k] < -32768 || ws[k] > 32767) R.in_range = false;
      }
      for (int y = 0; y < 8; ++y) {
        int32_t out[8];
        idct_1d(ws + 8 * y, out, 18);
        for (int k = 0; k < 8; ++k)
          if (out[k] < -512 || out[k] > 511) R.in_range = false;
      }
      const int64_t by = b / d.blocks_w[c], bx = b % d.blocks_w[c];
      for (int y = 0; y < 8; ++y) idct_row(ws, y, planes.get() + d.plane_off[c] + (by * 8 + y) * d.plane_w[c] + bx * 8);
    }
  }
  for (int y = 0; y < d.height; ++y)
    for (int x = 0; x < d.width; ++x) pixel_rgb(d, planes.get(), y, x, R.rgb.data() + ((size_t)y * d.width + x) * 3);
  return R;
}

static uint64_t rng_state = 1;
static uint32_t rnd() {                                          // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 2685821657736338717ull) >> 32);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: jpeg_core_check CASES [MUTATIONS_PER_FILE] [SEED]\n"); return 2; }
  const int per_file = argc > 2 ? atoi(argv[2]) : 0;
  rng_state = argc > 3 ? strtoull(argv[3], nullptr, 10) | 1 : 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> all;
  uint8_t chunk[65536];
  for (size_t k; (k = fread(chunk, 1, sizeof(chunk), f)) > 0;) all.insert(all.end(), chunk, chunk + k);
  fclose(f);
  size_t pos = 0;
  auto u32 = [&]() { uint32_t v = 0; if (pos + 4 <= all.size()) memcpy(&v, all.data() + pos, 4); pos += 4; return v; };
  const uint32_t count = u32();
  int failures = 0, mutated = 0, same = 0, flagged = 0, fallback = 0, changed = 0;
  int given = 0, given_fallback = 0, given_flagged = 0, given_unread = 0, given_equal = 0, given_wild = 0;
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t kind = u32(), nj = u32(), npx = u32();
    if (pos + nj + (size_t)npx > all.size()) { fprintf(stderr, "case %u: the case file is cut\n", k); return 2; }
    const uint8_t* jpg = all.data() + pos;
    const uint8_t* px = jpg + nj;
    pos += nj + (size_t)npx;
    const Result R = decode(jpg, nj);
    bool ok;
    if (kind == 0) ok = R.route == ROUTE_DEVICE && R.status == 0 && R.rgb.size() == npx && memcmp(R.rgb.data(), px, npx) == 0;
    else if (kind == 1) ok = R.route != ROUTE_DEVICE;
    else if (kind == 2) ok = R.route == ROUTE_DEVICE && R.status > 0;
    else {                                                       // a mutation written by the test: pixels as Pillow decodes it, if it can
      ok = R.route != ROUTE_DEVICE || R.status > 0 || npx == 0 || !R.in_range || (R.rgb.size() == npx && memcmp(R.rgb.data(), px, npx) == 0);
      ++given;
      if (R.route != ROUTE_DEVICE) ++given_fallback; else if (R.status) ++given_flagged; else if (npx == 0) ++given_unread;
      else if (!R.in_range) ++given_wild; else ++given_equal;
    }
    if (!ok) { ++failures; fprintf(stderr, "case %u (kind %u): route %d status %d, %zu pixel bytes against %u\n", k, kind, R.route, R.status, R.rgb.size(), npx); }
    if (kind != 0 || R.route != ROUTE_DEVICE) continue;
    Parsed P;
    parse(jpg, nj, &P);
    const size_t scan = P.segs.empty() ? nj : P.segs[0].begin;   // headers [0, scan), entropy data behind
    std::vector<uint8_t> m;
    for (int t = 0; t < per_file; ++t) {
      m.assign(jpg, jpg + nj);
      const uint32_t how = rnd() % 8;
      if (how < 2) m[rnd() % scan] = (uint8_t)rnd();                                     // a header byte (marker, length, table, frame)
      else if (how < 4 && scan < nj) m[scan + rnd() % (nj - scan)] = (uint8_t)rnd();     // an entropy byte
      else if (how < 6 && scan < nj) m[scan + rnd() % (nj - scan)] ^= (uint8_t)(1u << (rnd() % 8));
      else if (how == 6) m.resize(rnd() % nj);                                           // cut anywhere
      else m.resize(scan + (scan < nj ? rnd() % (nj - scan) : 0));                       // cut inside the scan
      const Result Q = decode(m.data(), m.size());
      ++mutated;
      if (Q.route != ROUTE_DEVICE) ++fallback;
      else if (Q.status) ++flagged;
      else if (Q.rgb == R.rgb) ++same;
      else ++changed;
    }
  }
  printf("cases %u failures %d | given-mutations %d: equal-to-Pillow %d flagged %d fallback %d Pillow-cannot-read %d beyond-range %d | mutations %d: same %d "
         "flagged %d fallback %d other-pixels %d\n", count, failures, given, given_equal, given_flagged, given_fallback, given_unread, given_wild, mutated,
         same, flagged, fallback, changed);
  return failures ? 1 : 0;
}
