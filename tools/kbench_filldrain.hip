// kbench_filldrain.hip -- what the 128 MiB float32 per-channel launch (config 2: 4096 rows of 1024 lane-vectors) pays ONCE,
// at its two ends, and which launch shape pays less.  Companion of kbench_timeline.hip (same arithmetic, same stamps); not
// part of the product.  Every launch is checked with hipGetLastError; a form that fails to launch is reported, never timed.
//
// A launch covers `units` four-vector tiles (256 lanes x 4 lane-vectors = 16 KiB in, 16 KiB out; a row is inner4 / 1024 of
// them).  A FORM says how the units are laid over workgroups:
//   G  256-lane groups per workgroup (workgroup = 256 * G threads; each group owns whole tiles, so its row stays wave-uniform)
//   K  tiles a group takes one after the other (second tile's loads behind the first tile's stores, no waits but the data's)
//   KS 0: the K tiles are adjacent units; 1: unit u and unit u + bulk / K
//   R  units at the END of the launch that run as finer tiles of UT lane-vectors per lane (4 / UT times as many groups)
//   P  odd multiplier that scatters the fine tiles' order (0 = in address order)
// and T512U2 / T1024U1: one row laid over a wider workgroup (lane stride 512 / 1024), the forms kbench_timeline.hip section D has.
//
// Per form, one run prints: the event-measured period over the cold ring of five buffer pairs (five interleaved repeats ->
// min / median), and from one stamped launch in the middle of a back-to-back series: when the last first-round workgroup
// entered, when the first tile retired, the retire rate in 0.5 us bins, and the time from 90 % of the bytes retired to the
// last store.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o tools/kbench_filldrain.bin tools/kbench_filldrain.hip
// Run:   tools/kbench_filldrain.bin [iters = 200] [rows = 4096] [inner4 = 1024]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

__device__ __forceinline__ float fq(float x, float s, float inv) {
  float q = __builtin_rintf(x * inv);
  q = fminf(fmaxf(q, -128.f), 127.f);
  return q * s;
}
__device__ __forceinline__ f4 fq4(f4 v, float s, float inv) {
  f4 r; r.x = fq(v.x, s, inv); r.y = fq(v.y, s, inv); r.z = fq(v.z, s, inv); r.w = fq(v.w, s, inv);
  return r;
}
__device__ __forceinline__ uint64_t now() { return __builtin_readsteadycounter(); }   // 100 MHz constant clock

struct Shape {
  uint32_t inner4;        // lane-vectors per row (a multiple of 1024)
  uint32_t upr;           // four-vector tiles (units) per row
  uint32_t bulk;          // units run as four-vector tiles
  uint32_t kstride;       // distance in units between a group's consecutive tiles
  uint32_t bulk_groups;   // groups that run bulk tiles
  uint32_t fine;          // fine tiles behind them
  uint32_t perm;          // odd multiplier of the fine tiles' order, 0 = none
};

// U lane-vectors of one row at vector offset `v0` (tile start + lane); stamps: s[0] entry (filled by the caller), s[1] loads landed,
// s[2] stores issued (LAST: completed)
template <int U, bool STAMP>
__device__ __forceinline__ void tile(const f4* __restrict__ x, f4* __restrict__ y, const float* __restrict__ scales, uint32_t row,
                                     uint64_t v0, uint64_t* s, bool last) {
  f4 v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(x + v0 + u * 256);
  const float sc = scales[row];
  const float inv = 1.0f / sc;
  if (STAMP) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (s) s[1] = now(); }
#pragma unroll
  for (int u = 0; u < U; ++u) __builtin_nontemporal_store(fq4(v[u], sc, inv), y + v0 + u * 256);
  if (STAMP) { if (last) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (s) s[2] = now(); }
}

// stamps: 3 per work item; work item of (group q, k) = q * K + k for bulk groups, bulk_groups * K + fine tile index behind them
template <int G, int K, int UT, bool STAMP>
__global__ __launch_bounds__(256 * G) void k_form(const float* __restrict__ xs, float* __restrict__ ys,
                                                  const float* __restrict__ scales, Shape sh, uint64_t* __restrict__ stamps) {
  uint64_t t0 = 0;
  if (STAMP) t0 = now();
  const f4* x = reinterpret_cast<const f4*>(xs);
  f4* y = reinterpret_cast<f4*>(ys);
  const uint32_t g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8), lane = threadIdx.x & 255;
  const uint32_t q = blockIdx.x * G + g;                     // group index over the launch (wave-uniform)
  if (q < sh.bulk_groups) {
    const uint32_t u0 = sh.kstride == 1 ? q * K : q;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t u = u0 + k * sh.kstride;
      if (u >= sh.bulk || (sh.kstride != 1 && k > 0 && q >= sh.kstride)) break;
      uint64_t* s = (STAMP && lane == 0) ? stamps + 3ull * (q * K + k) : nullptr;
      if (s) s[0] = k == 0 ? t0 : now();
      tile<4, STAMP>(x, y, scales, u / sh.upr, (uint64_t)u * 1024 + lane, s, k == K - 1);
    }
  } else {
    uint32_t t = q - sh.bulk_groups;
    if (t >= sh.fine) return;
    uint64_t* s = (STAMP && lane == 0) ? stamps + 3ull * ((uint64_t)sh.bulk_groups * K + t) : nullptr;
    if (s) s[0] = t0;
    if (sh.perm) t = (uint32_t)(((uint64_t)t * sh.perm) % sh.fine);
    constexpr uint32_t PARTS = 4 / UT;
    const uint32_t u = sh.bulk + t / PARTS, part = t % PARTS;
    tile<UT, STAMP>(x, y, scales, u / sh.upr, (uint64_t)u * 1024 + part * (UT * 256) + lane, s, true);
  }
}

// one row laid over a workgroup of T threads, U lane-vectors per lane at stride T (inner4 == T * U * tiles)
template <int T, int U, bool STAMP>
__global__ __launch_bounds__(T) void k_wide(const float* __restrict__ xs, float* __restrict__ ys, const float* __restrict__ scales,
                                            Shape sh, uint64_t* __restrict__ stamps) {
  uint64_t t0 = 0, t1 = 0;
  if (STAMP) t0 = now();
  const uint32_t tpr = sh.inner4 / (T * U);
  const uint32_t row = blockIdx.x / tpr, tl = blockIdx.x - row * tpr;
  const f4* x = reinterpret_cast<const f4*>(xs) + (uint64_t)row * sh.inner4 + tl * (T * U) + threadIdx.x;
  f4* y = reinterpret_cast<f4*>(ys) + (uint64_t)row * sh.inner4 + tl * (T * U) + threadIdx.x;
  f4 v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(x + u * T);
  const float sc = scales[row];
  const float inv = 1.0f / sc;
  if (STAMP) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); t1 = now(); }
#pragma unroll
  for (int u = 0; u < U; ++u) __builtin_nontemporal_store(fq4(v[u], sc, inv), y + u * T);
  if (STAMP) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if ((threadIdx.x & 255) == 0) {                            // one work item per 256 lanes, like the grouped forms
      uint64_t* p = stamps + 3ull * (blockIdx.x * (T / 256) + (threadIdx.x >> 8));
      p[0] = t0; p[1] = t1; p[2] = now();
    }
  }
}

struct Form {
  std::string name;
  int G, K, UT;            // UT 0: no fine tail
  int ks_split;            // K tiles: 0 adjacent, 1 at u and u + bulk / K
  uint32_t tail_units;     // R
  uint32_t perm;
  int wide;                // 0 grouped form, 512 / 1024: k_wide<T, 4096 / T / 4 ...>
};

typedef void (*kern_t)(const float*, float*, const float*, Shape, uint64_t*);
template <bool STAMP>
static kern_t pick(const Form& f) {
  if (f.wide == 512) return k_wide<512, 2, STAMP>;
  if (f.wide == 1024) return k_wide<1024, 1, STAMP>;
  const int ut = f.UT ? f.UT : 1;
#define PICK(G_, K_, UT_) if (f.G == G_ && f.K == K_ && ut == UT_) return k_form<G_, K_, UT_, STAMP>
  PICK(1, 1, 1); PICK(1, 1, 2); PICK(2, 1, 1); PICK(2, 1, 2); PICK(4, 1, 1); PICK(4, 1, 2);
  PICK(1, 2, 1); PICK(1, 2, 2); PICK(2, 2, 1); PICK(2, 2, 2);
#undef PICK
  return nullptr;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 200;
  const uint32_t ROWS = argc > 2 ? (uint32_t)atoi(argv[2]) : 4096;
  const uint32_t INNER4 = argc > 3 ? (uint32_t)atoi(argv[3]) : 1024;
  if (INNER4 % 1024 != 0 || ROWS == 0) { printf("inner4 must be a multiple of 1024\n"); return 2; }
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  printf("device %s CUs %d clock %d kHz; rows %u x %u lane-vectors (%.0f MiB in + out)\n", prop.name, prop.multiProcessorCount,
         prop.clockRate, ROWS, INNER4, 2.0 * ROWS * INNER4 * 16 / 1048576.0);
  const uint32_t upr = INNER4 / 1024, units = ROWS * upr;
  const uint32_t round = 8u * (uint32_t)prop.multiProcessorCount;      // resident 256-thread groups
  const int RING = 5;
  const size_t n = (size_t)ROWS * INNER4 * 4, bytes = n * 4;
  float *x[RING], *y[RING], *scales, *yref;
  std::vector<float> h(n);
  for (size_t i = 0; i < n; ++i) h[i] = (float)((i * 2654435761u) >> 8 & 0xffff) / 65536.f * 4.f - 2.f;
  std::vector<float> hs(ROWS);
  for (uint32_t i = 0; i < ROWS; ++i) hs[i] = (0.5f + (i % 97) / 97.f) / 64.f;
  for (int r = 0; r < RING; ++r) { CK(hipMalloc(&x[r], bytes)); CK(hipMalloc(&y[r], bytes)); CK(hipMemcpy(x[r], h.data(), bytes, hipMemcpyHostToDevice)); }
  CK(hipMalloc(&yref, bytes));
  CK(hipMalloc(&scales, ROWS * 4)); CK(hipMemcpy(scales, hs.data(), ROWS * 4, hipMemcpyHostToDevice));
  hipStream_t st; CK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));

  const uint32_t Q = round / 4;                                        // a quarter of a round of units
  std::vector<Form> forms = {
    {"shipped: G1 K1 (256 thr, one tile)", 1, 1, 0, 0, 0, 0, 0},
    {"fill a: T512 U2, one row per workgroup", 1, 1, 0, 0, 0, 0, 512},
    {"fill a: T1024 U1, one row per workgroup", 1, 1, 0, 0, 0, 0, 1024},
    {"fill a: G2 (512 thr, two tiles side by side)", 2, 1, 0, 0, 0, 0, 0},
    {"fill a: G4 (1024 thr, four tiles side by side)", 4, 1, 0, 0, 0, 0, 0},
    {"fill b: G1 K2 adjacent", 1, 2, 0, 0, 0, 0, 0},
    {"fill b: G1 K2 split (u, u + units/2)", 1, 2, 0, 1, 0, 0, 0},
    {"drain a: tail R=round/4 as U2", 1, 1, 2, 0, Q, 0, 0},
    {"drain a: tail R=round/4 as U1", 1, 1, 1, 0, Q, 0, 0},
    {"drain a: tail R=round/2 as U2", 1, 1, 2, 0, 2 * Q, 0, 0},
    {"drain a: tail R=round/2 as U1", 1, 1, 1, 0, 2 * Q, 0, 0},
    {"drain a: tail R=round as U2", 1, 1, 2, 0, 4 * Q, 0, 0},
    {"drain b: tail R=round/2 as U2, order x 37", 1, 1, 2, 0, 2 * Q, 37, 0},
    {"drain b: tail R=round/2 as U1, order x 37", 1, 1, 1, 0, 2 * Q, 37, 0},
    {"both: G2 + tail R=round/2 as U2", 2, 1, 2, 0, 2 * Q, 0, 0},
    {"both: G2 + tail R=round/2 as U1", 2, 1, 1, 0, 2 * Q, 0, 0},
    {"both: G4 + tail R=round/2 as U2", 4, 1, 2, 0, 2 * Q, 0, 0},
    {"both: K2 adjacent + tail R=round/2 as U2", 1, 2, 2, 0, 2 * Q, 0, 0},
    {"both: G2 K2 adjacent + tail R=round/2 as U2", 2, 2, 2, 0, 2 * Q, 0, 0},
  };
  if (upr != 1) forms.erase(std::remove_if(forms.begin(), forms.end(), [](const Form& f) { return f.wide != 0; }), forms.end());

  struct Plan { Shape sh; unsigned grid, threads; uint32_t items; kern_t plain, stamped; };
  std::vector<Plan> plans;
  for (const Form& f : forms) {
    Plan p{};
    p.plain = pick<false>(f); p.stamped = pick<true>(f);
    if (!p.plain || !p.stamped) { printf("form %s: not built\n", f.name.c_str()); return 2; }
    Shape& sh = p.sh;
    sh.inner4 = INNER4; sh.upr = upr;
    if (f.wide) {
      p.threads = f.wide; p.grid = ROWS * (INNER4 / 1024); p.items = p.grid * (f.wide / 256);
      sh.bulk = units; sh.kstride = 1; sh.bulk_groups = units; sh.fine = 0; sh.perm = 0;
    } else {
      const uint32_t tail = f.UT ? std::min(f.tail_units, units) : 0;
      sh.bulk = units - tail;
      sh.bulk_groups = (sh.bulk + f.K - 1) / f.K;
      sh.kstride = (f.K > 1 && f.ks_split) ? sh.bulk_groups : 1;
      sh.fine = f.UT ? tail * (4 / f.UT) : 0;
      sh.perm = f.perm;
      if (sh.perm) while (sh.fine && std::__gcd(sh.perm, sh.fine) != 1) sh.perm += 2;
      // bulk groups rounded up to whole workgroups so that a workgroup is all bulk or all fine
      const uint32_t bulk_wgs = (sh.bulk_groups + f.G - 1) / f.G, fine_wgs = (sh.fine + f.G - 1) / f.G;
      if (sh.fine && sh.bulk_groups % f.G != 0) { printf("form %s: bulk groups %u not a multiple of G\n", f.name.c_str(), sh.bulk_groups); return 2; }
      p.threads = 256 * f.G; p.grid = bulk_wgs + fine_wgs;
      p.items = sh.bulk_groups * f.K + sh.fine;
    }
    plans.push_back(p);
  }
  uint32_t max_items = 0;
  for (const Plan& p : plans) max_items = std::max(max_items, p.items);
  const int KL = 12;                                                   // stamped launches back to back; number KL / 2 is printed
  uint64_t* d_stamps; CK(hipMalloc(&d_stamps, (size_t)KL * max_items * 3 * 8));

  auto launch = [&](const Plan& p, bool stamp, int i, uint64_t* stamps, float* out) {
    hipLaunchKernelGGL(stamp ? p.stamped : p.plain, dim3(p.grid), dim3(p.threads), 0, st, x[i % RING], out ? out : y[i % RING], scales, p.sh, stamps);
  };
  // pre-warm (clocks), then the reference output of the shipped form
  for (int i = 0; i < 3000; ++i) launch(plans[0], false, i, nullptr, nullptr);
  CK(hipStreamSynchronize(st));
  launch(plans[0], false, 0, nullptr, yref);
  CK(hipStreamSynchronize(st)); CK(hipGetLastError());
  std::vector<float> ref(n), got(n);
  CK(hipMemcpy(ref.data(), yref, bytes, hipMemcpyDeviceToHost));

  // ---- periods: five interleaved repeats over all forms ----
  const int REPS = 5;
  std::vector<std::vector<double>> per(plans.size());
  std::vector<int> ok(plans.size(), 1);
  for (int rep = 0; rep < REPS; ++rep)
    for (size_t f = 0; f < plans.size(); ++f) {
      if (!ok[f]) continue;
      for (int i = 0; i < 20; ++i) launch(plans[f], false, i, nullptr, nullptr);
      CK(hipStreamSynchronize(st));
      CK(hipEventRecord(e0, st));
      for (int i = 0; i < iters; ++i) launch(plans[f], false, i, nullptr, nullptr);
      CK(hipEventRecord(e1, st));
      CK(hipEventSynchronize(e1));
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) { printf("%s FAILED to launch: %s\n", forms[f].name.c_str(), hipGetErrorString(e)); ok[f] = 0; continue; }
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      per[f].push_back(ms * 1000.0 / iters);
    }
  printf("\n[periods] cold ring of %d pairs, %d launches per repeat, %d interleaved repeats; outputs compared with the shipped form\n", RING, iters, REPS);
  std::vector<double> med(plans.size(), 0.0);
  for (size_t f = 0; f < plans.size(); ++f) {
    if (!ok[f]) continue;
    CK(hipMemset(y[0], 0, bytes));
    launch(plans[f], false, 0, nullptr, nullptr);
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(got.data(), y[0], bytes, hipMemcpyDeviceToHost));
    const bool same = memcmp(got.data(), ref.data(), bytes) == 0;
    std::vector<double> v = per[f]; std::sort(v.begin(), v.end());
    med[f] = v[v.size() / 2];
    printf("  %-46s grid %5u x %4u  min %6.2f  median %6.2f  max %6.2f us  (%5.0f GB/s, %+5.2f %% vs shipped)  equal=%s\n", forms[f].name.c_str(),
           plans[f].grid, plans[f].threads, v.front(), med[f], v.back(), 2.0 * bytes / med[f] / 1e3, (med[f] / med[0] - 1.0) * 100.0, same ? "yes" : "NO");
  }

  // ---- timelines ----
  for (size_t f = 0; f < plans.size(); ++f) {
    if (!ok[f]) continue;
    const Plan& p = plans[f];
    CK(hipMemset(d_stamps, 0, (size_t)KL * max_items * 3 * 8));
    for (int i = 0; i < 20; ++i) launch(p, true, i, d_stamps, nullptr);
    CK(hipStreamSynchronize(st));
    CK(hipMemset(d_stamps, 0, (size_t)KL * max_items * 3 * 8));
    CK(hipEventRecord(e0, st));
    for (int i = 0; i < KL; ++i) launch(p, true, i, d_stamps + (size_t)i * max_items * 3, nullptr);
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<uint64_t> hst((size_t)KL * max_items * 3);
    CK(hipMemcpy(hst.data(), d_stamps, hst.size() * 8, hipMemcpyDeviceToHost));
    const uint32_t bulk_items = forms[f].wide ? p.items : p.sh.bulk_groups * forms[f].K;
    const double fine_bytes = forms[f].UT ? forms[f].UT * 4096.0 : 0.0;
    std::vector<double> spans, bubbles, fills, firsts, drains;
    uint64_t prev_end = 0;
    for (int k = 0; k < KL; ++k) {
      const uint64_t* s = hst.data() + (size_t)k * max_items * 3;
      uint64_t mn = ~0ull, mx = 0;
      std::vector<uint64_t> entries;                                   // of workgroups' first groups: item q * K, q % G == 0
      std::vector<std::pair<uint64_t, double>> done;                   // (retire stamp, bytes written)
      double total = 0;
      for (uint32_t it = 0; it < p.items; ++it) {
        if (!s[3 * it + 2]) continue;                                  // a guarded-out tile of a ragged grid
        mn = std::min(mn, s[3 * it]); mx = std::max(mx, s[3 * it + 2]);
        const double b = forms[f].wide ? 16384.0 * 256 / forms[f].wide : (it < bulk_items ? 16384.0 : fine_bytes);
        done.push_back({s[3 * it + 2], b}); total += b;
        const bool first_of_wg = forms[f].wide ? it % (forms[f].wide / 256) == 0
                                 : (it < bulk_items ? (it % forms[f].K == 0 && (it / forms[f].K) % forms[f].G == 0) : (it - bulk_items) % forms[f].G == 0);
        if (first_of_wg) entries.push_back(s[3 * it]);
      }
      std::sort(entries.begin(), entries.end()); std::sort(done.begin(), done.end());
      const uint32_t wg_groups = forms[f].wide ? forms[f].wide / 256 : forms[f].G;
      const size_t first_round = std::min<size_t>(entries.size(), round / wg_groups);
      spans.push_back((mx - mn) * 0.01);
      fills.push_back((entries[first_round - 1] - mn) * 0.01);
      firsts.push_back((done.front().first - mn) * 0.01);
      double acc = 0; uint64_t t90 = mx;
      for (auto& d : done) { acc += d.second; if (acc >= 0.9 * total) { t90 = d.first; break; } }
      drains.push_back((mx - t90) * 0.01);
      if (k) bubbles.push_back(((double)mn - (double)prev_end) * 0.01);
      prev_end = mx;
      if (k == KL / 2) {
        printf("\n[timeline] %s: launch %d of %d back to back (event period of the stamped series %.2f us; plain median %.2f us)\n",
               forms[f].name.c_str(), k, KL, ms * 1000.0 / KL, med[f]);
        printf("    retired per 0.5 us bin, GB/s written (x2 = traffic):");
        size_t j = 0;
        for (double t = 0.5; t < (mx - mn) * 0.01 + 0.5; t += 0.5) {
          const uint64_t lim = mn + (uint64_t)(t * 100.0);
          double b = 0;
          while (j < done.size() && done[j].first <= lim) b += done[j++].second;
          printf(" %4.0f", b / 0.5e-6 / 1e9);
        }
        printf("\n");
      }
    }
    auto m = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    printf("    medians over %d launches: last first-round workgroup entered %.2f us | first tile retired %.2f us | 90 %% of bytes retired -> last store %.2f us"
           " | span %.2f us | bubble to the next launch %.2f us\n", KL, m(fills), m(firsts), m(drains), m(spans), m(bubbles));
  }
  return 0;
}
