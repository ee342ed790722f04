// Host program over calciumgan_amd/csrc/fft_stages.h as the kernels include it
// (tests/test_fft_stages_host.py builds it with the address and undefined-
// behaviour sanitizers and runs it as a child process):
//   fft_stages_host check
//       every structural property the kernels of ifft.hip, windows.hip and
//       trace_psd.hip rely on, for every T = 32 .. 8192 with their G =
//       ifft_group(T) and rows_mask = 32 / G - 1; prints one line per T and
//       exits 0, or names the first failed check and exits 1
//   fft_stages_host ifft T n in.bin out.bin
//       the whole schedule, one butterfly after the other, on n complex float32
//       traces of T bins ([n][T][re, im]): the inverse transform, scaled by 1 / T
//       and in time order, written in the same layout
// The order of the stages (fft_for_each_stage), a lane's walk through a stage
// (fft_stage) and the driver (fft_run_stages) are the header's, the ones the
// kernels call; fft_run_stages<1, 1> with lane 0 is the schedule one butterfly
// after the other.
// A butterfly holds pointers into the image, so the image lies in the middle of
// an arena three images long: an index up to one image out of range is seen by
// the range check here, anything further by the sanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fft_stages.h"

namespace {

int fail(const char* what, int T, long long at) {
  std::fprintf(stderr, "FAILED: %s (T = %d, at %lld)\n", what, T, at);
  return 1;
}

struct Geometry {
  int T, G, rows_mask, odd, elems;
  explicit Geometry(int T_)
      : T(T_), G(ifft_group(T_)), rows_mask(32 / ifft_group(T_) - 1),
        odd(__builtin_ctz((unsigned)T_) & 1), elems(T_ * ifft_group(T_)) {}
};

// e^{+2 pi i k / T}, k < T / 4, in float64 rounded once to float32
std::vector<cf32> twiddles(int T) {
  std::vector<cf32> tw(T / 4);
  for (int k = 0; k < T / 4; ++k) {
    const double a = 2.0 * M_PI * (double)k / (double)T;
    tw[k] = cf32{(float)std::cos(a), (float)std::sin(a)};
  }
  return tw;
}

struct Image {
  std::vector<cf32> arena;
  cf32* buf;
  explicit Image(int elems) : arena(3 * (size_t)elems, cf32{0.f, 0.f}),
                              buf(arena.data() + elems) {}
};

// butterfly idx of a stage, as a lane of any of the three kernels loads it
int load(IfftBfly& f, cf32* buf, const Geometry& s, int N, int idx) {
  const int gshift = __builtin_ctz((unsigned)s.G);
  const int j = idx >> gshift, g = idx & (s.G - 1);
  if (N == 0) {
    ifft_radix2_load(f, buf, s.T, s.G, s.rows_mask, j, g);
    return 2;
  }
  ifft_radix4_load(f, buf, s.G, s.rows_mask, N, j, g);
  return 4;
}

// the schedule as a workgroup of THREADS lanes with batches of BATCH runs it:
// stage by stage and, within a stage, lane by lane
template <int THREADS, int BATCH>
void run_stages_by_lanes(cf32* buf, const cf32* tw, const Geometry& s) {
  fft_for_each_stage(s.T, s.odd, [&](int stage) {
    for (int lane = 0; lane < THREADS; ++lane)
      fft_stage<THREADS, BATCH>(buf, tw, s.T, s.G, s.rows_mask, stage, lane);
  });
}

// a fixed pseudo-random image: 24 bits of a linear congruential generator per
// component, in [-1, 1)
void fill_pattern(cf32* buf, int elems) {
  unsigned state = 12345u;
  auto next = [&state] {
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) * (1.0f / 8388608.0f) - 1.0f;
  };
  for (int e = 0; e < elems; ++e) {
    buf[e].re = next();
    buf[e].im = next();
  }
}

// the first element whose bytes differ, or -1
long long first_difference(const cf32* a, const cf32* b, int elems) {
  for (int e = 0; e < elems; ++e)
    if (std::memcmp(a + e, b + e, sizeof(cf32))) return e;
  return -1;
}

// log2(T) eta of tests/ifft_cases.py: higham_bound
double higham_bound(int T) {
  const double u = std::ldexp(1.0, -24), mu = 2 * u, gamma4 = 4 * u / (1 - 4 * u);
  return std::log2((double)T) * (mu + gamma4 * (std::sqrt(2.0) + mu));
}

int check(int T) {
  const Geometry s(T);
  const int G = s.G, M = 32 / G;
  if (G != (kIfftTraceElems / T < kIfftMaxGroup ? kIfftTraceElems / T : kIfftMaxGroup))
    return fail("G = min(16, 8192 / T)", T, G);
  if (s.rows_mask != M - 1) return fail("rows_mask = 32 / G - 1", T, s.rows_mask);

  // ifft_phys is a bijection of [0, T)
  std::vector<int> seen(T, 0);
  for (int t = 0; t < T; ++t) {
    const int p = ifft_phys(t, s.rows_mask);
    if (p < 0 || p >= T) return fail("ifft_phys stays inside [0, T)", T, t);
    seen.at(p) += 1;
  }
  for (int p = 0; p < T; ++p)
    if (seen.at(p) != 1) return fail("ifft_phys is a bijection", T, p);

  // ifft_row_of_time inverts ifft_time_of_row; bit 1 of a row is clear exactly
  // when its bin is below T / 2; row 2 holds bin T / 2
  std::fill(seen.begin(), seen.end(), 0);
  for (int p = 0; p < T; ++p) {
    const int u = ifft_time_of_row(p, T, s.odd);
    if (u < 0 || u >= T) return fail("ifft_time_of_row stays inside [0, T)", T, p);
    seen.at(u) += 1;
    if (ifft_row_of_time(u, T, s.odd) != p)
      return fail("ifft_row_of_time inverts ifft_time_of_row", T, p);
    if (((p & 2) == 0) != (u < T / 2))
      return fail("bit 1 of a row is clear iff its bin is below T / 2", T, p);
  }
  for (int u = 0; u < T; ++u) {
    if (seen.at(u) != 1) return fail("ifft_time_of_row is a bijection", T, u);
    if (ifft_time_of_row(ifft_row_of_time(u, T, s.odd), T, s.odd) != u)
      return fail("ifft_time_of_row inverts ifft_row_of_time", T, u);
  }
  if (ifft_time_of_row(2, T, s.odd) != T / 2)
    return fail("row 2 holds bin T / 2", T, 2);

  // psd_low_row(j), j < T / 2, lists every row of a bin below T / 2 once, and
  // the mirror-row table of trace_psd.hip stays inside [0, T) and holds the
  // row of bin T - u
  std::fill(seen.begin(), seen.end(), 0);
  for (int j = 0; j < T / 2; ++j) {
    const int p = psd_low_row(j);
    if (p < 0 || p >= T) return fail("psd_low_row stays inside [0, T)", T, j);
    if (p & 2) return fail("psd_low_row lists rows of bins below T / 2", T, j);
    seen.at(p) += 1;
    const int u = ifft_time_of_row(p, T, s.odd);
    const int mirror = ifft_row_of_time((T - u) & (T - 1), T, s.odd);
    const int m = ifft_phys(mirror, s.rows_mask);
    if (m < 0 || m >= T || m > 0xffff)
      return fail("the mirror-row table stays inside [0, T)", T, j);
    if (ifft_time_of_row(mirror, T, s.odd) != ((T - u) & (T - 1)))
      return fail("the mirror row holds bin T - u", T, j);
  }
  for (int p = 0; p < T; ++p)
    if (seen.at(p) != ((p & 2) ? 0 : 1))
      return fail("psd_low_row lists each row of a bin below T / 2 once", T, p);

  // every stage: the butterflies' elements lie inside the image, are pairwise
  // disjoint and cover it (no barrier separates the butterflies of a stage)
  Image image(s.elems);
  std::vector<int> touched(s.elems);
  std::vector<int> stages;
  fft_for_each_stage(T, s.odd, [&](int N) { stages.push_back(N); });
  for (int N : stages) {
    std::fill(touched.begin(), touched.end(), 0);
    const int legs = N == 0 ? 2 : 4, count = s.elems / legs;
    for (int idx = 0; idx < count; ++idx) {
      IfftBfly f;
      if (load(f, image.buf, s, N, idx) != legs) return fail("legs", T, N);
      for (int k = 0; k < legs; ++k) {
        const long long e = f.p[k] - image.buf;
        if (e < 0 || e >= s.elems)
          return fail("a butterfly's elements lie inside the image", T,
                      (long long)N * 100000 + idx);
        touched.at((size_t)e) += 1;
      }
    }
    for (int e = 0; e < s.elems; ++e)
      if (touched.at(e) != 1)
        return fail("a stage's butterflies are disjoint and cover the image", T,
                    (long long)N * 100000 + e);

    // the 32 lanes of an LDS lane group hold M butterflies of consecutive j:
    // every leg's M rows lie on M distinct bank positions (row mod M)
    const int gshift = __builtin_ctz((unsigned)G);
    for (int j0 = 0; j0 + M <= (count >> gshift); j0 += M)
      for (int k = 0; k < legs; ++k) {
        unsigned banks = 0;
        for (int j = j0; j < j0 + M; ++j) {
          IfftBfly f;
          load(f, image.buf, s, N, j << gshift);
          banks |= 1u << (((f.p[k] - image.buf) >> gshift) & (M - 1));
        }
        if (banks != (M == 32 ? 0xffffffffu : (1u << M) - 1))
          return fail("a lane group's rows lie on distinct bank positions", T,
                      (long long)N * 100000 + j0);
      }
  }
  // (the row-order walks of load and store: M consecutive rows)
  for (int t0 = 0; t0 < T; t0 += M) {
    unsigned banks = 0;
    for (int t = t0; t < t0 + M; ++t)
      banks |= 1u << (ifft_phys(t, s.rows_mask) & (M - 1));
    if (banks != (M == 32 ? 0xffffffffu : (1u << M) - 1))
      return fail("a row-order walk lies on distinct bank positions", T, t0);
  }

  // the schedule on one-hot bins k0 (a real 1 in column 0, an imaginary 1 in
  // the last column): e^{2 pi i k0 t / T} in float64, under Higham's bound
  const std::vector<cf32> tw = twiddles(T);
  const int ks[] = {1, T / 4 + 1, T / 2 - 1, T / 2, T - 1};
  double worst = 0.0;
  for (int k0 : ks) {
    for (int e = 0; e < s.elems; ++e) image.buf[e] = cf32{0.f, 0.f};
    image.buf[ifft_phys(k0, s.rows_mask) * G + 0].re = 1.f;
    image.buf[ifft_phys(k0, s.rows_mask) * G + (G - 1)].im += 1.f;
    fft_run_stages<1, 1>(image.buf, tw.data(), T, G, s.rows_mask, s.odd, 0);
    double err0 = 0.0, err1 = 0.0;
    for (int p = 0; p < T; ++p) {
      const int t = ifft_time_of_row(p, T, s.odd);
      const double a = 2.0 * M_PI * (double)(((long long)k0 * t) % T) / (double)T;
      double wr[2] = {std::cos(a), -std::sin(a)}, wi[2] = {std::sin(a), std::cos(a)};
      if (G == 1) {  // one column holds 1 + i
        wr[0] += wr[1];
        wi[0] += wi[1];
      }
      const cf32 c0 = image.buf[ifft_phys(p, s.rows_mask) * G + 0];
      err0 += (c0.re - wr[0]) * (c0.re - wr[0]) + (c0.im - wi[0]) * (c0.im - wi[0]);
      if (G > 1) {
        const cf32 c1 = image.buf[ifft_phys(p, s.rows_mask) * G + (G - 1)];
        err1 += (c1.re - wr[1]) * (c1.re - wr[1]) + (c1.im - wi[1]) * (c1.im - wi[1]);
      }
    }
    // ||y64||^2 = T (2 T where the column holds 1 + i)
    const double e0 = std::sqrt(err0 / (G == 1 ? 2.0 * T : (double)T));
    const double e1 = std::sqrt(err1 / (double)T);
    worst = std::fmax(worst, std::fmax(e0, e1));
    if (!(e0 <= higham_bound(T)) || !(e1 <= higham_bound(T)))
      return fail("the schedule on a one-hot bin is the float64 transform", T, k0);
  }

  // the lanes of a workgroup run every butterfly of a stage exactly once: the
  // schedule walked as the kernels' lanes walk it (ifft.hip and windows.hip;
  // trace_psd.hip, whose written-out copy of the walk has fft_stage's guards
  // and strides) leaves the bytes that one butterfly after the other leaves
  // (a stage's butterflies are disjoint: a butterfly skipped or repeated shows)
  static_assert(kWinFftThreads == kIfftThreads && kWinBflyBatch == kIfftBflyBatch,
                "windows.hip walks a stage as ifft.hip does: one run covers both");
  Image wide(s.elems), narrow(s.elems);
  fill_pattern(image.buf, s.elems);
  fill_pattern(wide.buf, s.elems);
  fill_pattern(narrow.buf, s.elems);
  fft_run_stages<1, 1>(image.buf, tw.data(), T, G, s.rows_mask, s.odd, 0);
  run_stages_by_lanes<kIfftThreads, kIfftBflyBatch>(wide.buf, tw.data(), s);
  run_stages_by_lanes<kPsdThreads, kPsdBflyBatch>(narrow.buf, tw.data(), s);
  long long at = first_difference(image.buf, wide.buf, s.elems);
  if (at >= 0)
    return fail("the lanes of ifft.hip and windows.hip run the schedule", T, at);
  at = first_difference(image.buf, narrow.buf, s.elems);
  if (at >= 0) return fail("the lanes of trace_psd.hip run the schedule", T, at);

  std::printf("T %5d  G %2d  rows_mask %2d  stages %d  one-hot max e %.3g  "
              "Higham bound %.3g  lane walks %dx%d %dx%d equal\n", T, G, s.rows_mask,
              (int)stages.size(), worst, higham_bound(T), kIfftThreads,
              kIfftBflyBatch, kPsdThreads, kPsdBflyBatch);
  return 0;
}

int transform(int T, int n, const char* in_path, const char* out_path) {
  if (!fft_length_ok(T) || n < 1) return fail("arguments", T, n);
  const Geometry s(T);
  std::vector<float> x((size_t)n * T * 2), y((size_t)n * T * 2);
  std::FILE* in = std::fopen(in_path, "rb");
  if (!in || std::fread(x.data(), sizeof(float), x.size(), in) != x.size())
    return fail("reading the input", T, n);
  std::fclose(in);
  const std::vector<cf32> tw = twiddles(T);
  Image image(s.elems);
  const float inv_T = 1.0f / (float)T;
  for (int c0 = 0; c0 < n; c0 += s.G) {
    for (int t = 0; t < T; ++t)
      for (int g = 0; g < s.G; ++g) {
        cf32 v{0.f, 0.f};
        if (c0 + g < n) {
          v.re = x.at(((size_t)(c0 + g) * T + t) * 2);
          v.im = x.at(((size_t)(c0 + g) * T + t) * 2 + 1);
        }
        image.buf[ifft_phys(t, s.rows_mask) * s.G + g] = v;
      }
    fft_run_stages<1, 1>(image.buf, tw.data(), T, s.G, s.rows_mask, s.odd, 0);
    for (int p = 0; p < T; ++p) {
      const int t = ifft_time_of_row(p, T, s.odd);
      for (int g = 0; g < s.G && c0 + g < n; ++g) {
        const cf32 v = image.buf[ifft_phys(p, s.rows_mask) * s.G + g];
        y.at(((size_t)(c0 + g) * T + t) * 2) = v.re * inv_T;
        y.at(((size_t)(c0 + g) * T + t) * 2 + 1) = v.im * inv_T;
      }
    }
  }
  std::FILE* out = std::fopen(out_path, "wb");
  if (!out || std::fwrite(y.data(), sizeof(float), y.size(), out) != y.size())
    return fail("writing the output", T, n);
  std::fclose(out);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "check")) {
    for (int T = kFftMinT; T <= kFftMaxT; T *= 2)
      if (check(T)) return 1;
    std::printf("all checks passed\n");
    return 0;
  }
  if (argc == 6 && !std::strcmp(argv[1], "ifft"))
    return transform(std::atoi(argv[2]), std::atoi(argv[3]), argv[4], argv[5]);
  std::fprintf(stderr, "usage: %s check | ifft T n in.bin out.bin\n", argv[0]);
  return 2;
}
