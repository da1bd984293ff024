// libsrk runtime: error reporting, per-device constant tables, srk_init.
//
// The tables are built on the host in double precision from the same closed forms the
// reference evaluates with numpy/scipy/librosa, then uploaded once per device:
//  * fbank triangles       models/model_fbanks_cnn.py:46-59 (rebuilt per call there)
//  * Slaney mel (norm=1)   librosa.filters.mel as called by model_mfcc_bgru.py:13
//  * DCT-II ortho [:13]    librosa.filters.dct / scipy.fftpack.dct(norm='ortho')
//  * windows               np.hamming(400) (model_fbanks_cnn.py:41), periodic Hann(640)
//                          (librosa stft), periodic Tukey(640, 0.25) (scipy spectrogram)
#include <atomic>
#include <functional>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <mutex>
#include <vector>

#include "gru_internal.h"
#include "srk_internal.h"

namespace srk {

// The plain options' variables with their defaults (options.h), then what the hooked ones store.
#define SRK_DEFINE_OPTION(type, var, name, accepts, def, doc) type var = def;
#define SRK_HOOKED_OPTION(name, hook, accepts, def, doc)
SRK_OPTION_LIST(SRK_DEFINE_OPTION, SRK_HOOKED_OPTION)
#undef SRK_DEFINE_OPTION
#undef SRK_HOOKED_OPTION
static std::atomic<int> g_opt_matmul_prec{kPrecF32};
thread_local int t_prec_override = -1;
int matmul_prec() { return t_prec_override >= 0 ? t_prec_override : g_opt_matmul_prec.load(std::memory_order_relaxed); }
unsigned long long* g_opt_gru_trace = nullptr;
unsigned g_opt_gru_dc_offset = 200;
int g_opt_gru_dwhh_fused = 1;
std::atomic<int64_t> g_scratch_gen{0};

ScratchPool* ScratchPool::head_ = nullptr;

int ScratchPool::get(size_t floats, float** out) {
  int dev = 0;
  SRK_CHECK_HIP(hipGetDevice(&dev));
  SRK_REQUIRE(dev >= 0 && dev < 64, SRK_ERR_INVALID, "device out of range");
  std::lock_guard<std::mutex> lk(mu_);
  Slot& s = slots_[dev];
  if (s.floats < floats) {   // grow-only: steady state never allocates
    if (float* old = s.p) {
      SRK_CHECK_HIP(hipDeviceSynchronize());
      s = Slot{};
      SRK_CHECK_HIP(hipFree(old));
    }
    const size_t want = floats + floats / 4;
    float* p = nullptr;
    SRK_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(float)));
    s = Slot{p, want};
    g_scratch_gen.fetch_add(1);
  }
  *out = s.p;
  return SRK_OK;
}

int ScratchPool::release_all() {
  SRK_CHECK_HIP(hipDeviceSynchronize());
  for (ScratchPool* pool = head_; pool; pool = pool->next_) {
    std::lock_guard<std::mutex> lk(pool->mu_);
    for (Slot& s : pool->slots_) {
      float* old = s.p;
      s = Slot{};
      if (old) SRK_CHECK_HIP(hipFree(old));
    }
  }
  g_scratch_gen.fetch_add(1);
  return SRK_OK;
}

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

namespace {

constexpr int kMaxDevices = 64;
DeviceTables g_tables[kMaxDevices];
std::mutex g_mutex;

template <class T>
int upload(T** dst, const std::vector<T>& src) {
  SRK_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(dst), src.size() * sizeof(T)));
  SRK_CHECK_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return SRK_OK;
}

std::vector<double> linspace(double a, double b, int n) {   // numpy.linspace semantics
  std::vector<double> y(n);
  const double step = (b - a) / (n - 1);
  for (int i = 0; i < n; ++i) y[i] = i * step + a;
  y[n - 1] = b;
  return y;
}

std::vector<float2> twiddles(int m, int count) {
  std::vector<float2> t(count);
  for (int k = 0; k < count; ++k) {
    const double a = -2.0 * M_PI * (double)k / (double)m;
    t[k] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  return t;
}

// Dense [nf][nbins] -> fixed-width windows: lo[m] (clamped so lo + width <= nbins) and
// w[m][q] = dense[m][lo + q] (zero outside the filter).  Every filter here spans <= 15 bins.
int to_windows(const std::vector<double>& w, int nf, int nbins, int width, std::vector<int>& lo,
               std::vector<float>& vals) {
  lo.assign(nf, 0);
  vals.assign((size_t)nf * width, 0.f);
  for (int m = 0; m < nf; ++m) {
    int first = -1, last = -1;
    for (int k = 0; k < nbins; ++k)
      if (w[(size_t)m * nbins + k] != 0.0) { if (first < 0) first = k; last = k; }
    if (first < 0) continue;
    SRK_REQUIRE(last - first + 1 <= width, SRK_ERR_INTERNAL, "filter %d wider than %d bins", m, width);
    const int l = std::min(first, nbins - width);
    lo[m] = l;
    for (int k = first; k <= last; ++k) vals[(size_t)m * width + (k - l)] = (float)w[(size_t)m * nbins + k];
  }
  return SRK_OK;
}

// Dense [nf][nbins] matrix -> CSR by filter (each filter is one contiguous run of bins).
void to_csr(const std::vector<double>& w, int nf, int nbins, std::vector<int>& lo,
            std::vector<int>& cnt, std::vector<int>& off, std::vector<float>& vals) {
  lo.assign(nf, 0); cnt.assign(nf, 0); off.assign(nf, 0); vals.clear();
  for (int m = 0; m < nf; ++m) {
    int first = -1, last = -1;
    for (int k = 0; k < nbins; ++k)
      if (w[(size_t)m * nbins + k] != 0.0) { if (first < 0) first = k; last = k; }
    off[m] = (int)vals.size();
    if (first < 0) continue;
    lo[m] = first; cnt[m] = last - first + 1;
    for (int k = first; k <= last; ++k) vals.push_back((float)w[(size_t)m * nbins + k]);
  }
}

// Dense [nf][nbins] -> lane pairs (filter l, filter nf-1-l), l < ceil(nf/2): meta {lo_a, cnt_a,
// lo_b, cnt_b} and the two weight runs back to back, zero padded to `taps`.
int to_pairs(const std::vector<double>& w, int nf, int nbins, int taps, std::vector<int4>& meta,
             std::vector<float>& vals) {
  const int np = (nf + 1) / 2;
  meta.assign(np, int4{0, 0, 0, 0});
  vals.assign((size_t)np * taps, 0.f);
  auto run = [&](int m, int& lo, int& cnt) {
    int first = -1, last = -1;
    for (int k = 0; k < nbins; ++k)
      if (w[(size_t)m * nbins + k] != 0.0) { if (first < 0) first = k; last = k; }
    lo = first < 0 ? 0 : first;
    cnt = first < 0 ? 0 : last - first + 1;
  };
  for (int l = 0; l < np; ++l) {
    int la, ca, lb = 0, cb = 0;
    run(l, la, ca);
    if (nf - 1 - l != l) run(nf - 1 - l, lb, cb);
    SRK_REQUIRE(ca + cb <= taps, SRK_ERR_INTERNAL, "filter pair %d spans %d > %d taps", l, ca + cb, taps);
    meta[l] = int4{la, ca, lb, cb};
    for (int q = 0; q < ca; ++q) vals[(size_t)l * taps + q] = (float)w[(size_t)l * nbins + la + q];
    for (int q = 0; q < cb; ++q) vals[(size_t)l * taps + ca + q] = (float)w[(size_t)(nf - 1 - l) * nbins + lb + q];
  }
  return SRK_OK;
}

// models/model_fbanks_cnn.py:48-50: the 122 mel points in Hz
std::vector<double> fbank_hz() {
  const int nfilt = 120, sr = 16000;
  const double high = 2595.0 * std::log10(1.0 + (sr / 2.0) / 700.0);
  std::vector<double> mel = linspace(0.0, high, nfilt + 2), hz(nfilt + 2);
  for (int i = 0; i < nfilt + 2; ++i) hz[i] = 700.0 * (std::pow(10.0, mel[i] / 2595.0) - 1.0);
  return hz;
}

// models/model_fbanks_cnn.py:46-59
std::vector<double> fbank_matrix() {
  const int nfilt = 120, nfft = 512, sr = 16000, nb = nfft / 2 + 1;
  const std::vector<double> hz = fbank_hz();
  std::vector<double> bin(nfilt + 2);
  for (int i = 0; i < nfilt + 2; ++i) bin[i] = std::floor((nfft + 1) * hz[i] / sr);
  std::vector<double> fb((size_t)nfilt * nb, 0.0);
  for (int m = 1; m <= nfilt; ++m) {
    const int fl = (int)bin[m - 1], fc = (int)bin[m], fr = (int)bin[m + 1];
    for (int k = fl; k < fc; ++k) fb[(size_t)(m - 1) * nb + k] = (k - bin[m - 1]) / (bin[m] - bin[m - 1]);
    for (int k = fc; k < fr; ++k) fb[(size_t)(m - 1) * nb + k] = (bin[m + 1] - k) / (bin[m + 1] - bin[m]);
  }
  return fb;
}

double hz_to_mel(double f) {   // Slaney (htk=False)
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
  const double logstep = std::log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
  const double logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// librosa.filters.mel(16000, 640, n_mels=128, norm=1)
std::vector<double> slaney_mel() {
  const int nmel = 128, nb = 321;
  std::vector<double> fft = linspace(0.0, 8000.0, nb);
  std::vector<double> mels = linspace(hz_to_mel(0.0), hz_to_mel(8000.0), nmel + 2), mf(nmel + 2);
  for (int i = 0; i < nmel + 2; ++i) mf[i] = mel_to_hz(mels[i]);
  std::vector<double> w((size_t)nmel * nb, 0.0);
  for (int i = 0; i < nmel; ++i) {
    const double fd0 = mf[i + 1] - mf[i], fd1 = mf[i + 2] - mf[i + 1];
    const double enorm = 2.0 / (mf[i + 2] - mf[i]);
    for (int k = 0; k < nb; ++k) {
      const double lower = -(mf[i] - fft[k]) / fd0, upper = (mf[i + 2] - fft[k]) / fd1;
      w[(size_t)i * nb + k] = std::max(0.0, std::min(lower, upper)) * enorm;
    }
  }
  return w;
}

int build_tables(DeviceTables& t) {
  int rc;
  if ((rc = upload(&t.tw256, twiddles(256, 256)))) return rc;
  if ((rc = upload(&t.tw320, twiddles(320, 320)))) return rc;
  if ((rc = upload(&t.post512, twiddles(512, 257)))) return rc;
  if ((rc = upload(&t.post640, twiddles(640, 321)))) return rc;

  std::vector<double> ham(400), hann(640), tuk(641);
  for (int n = 0; n < 400; ++n) ham[n] = 0.54 - 0.46 * std::cos(2.0 * M_PI * n / 399.0);
  for (int n = 0; n < 640; ++n) hann[n] = 0.5 - 0.5 * std::cos(2.0 * M_PI * n / 640.0);
  {  // scipy tukey(641, 0.25, sym=True)[:640]
    const int m = 641;
    const double alpha = 0.25;
    const int width = (int)std::floor(alpha * (m - 1) / 2.0);
    for (int n = 0; n < m; ++n) tuk[n] = 1.0;
    for (int n = 0; n <= width; ++n)
      tuk[n] = 0.5 * (1.0 + std::cos(M_PI * (-1.0 + 2.0 * n / alpha / (m - 1))));
    for (int n = m - width - 1; n < m; ++n)
      tuk[n] = 0.5 * (1.0 + std::cos(M_PI * (-2.0 / alpha + 1.0 + 2.0 * n / alpha / (m - 1))));
    tuk.resize(640);
  }
  double s2 = 0.0;
  for (double v : tuk) s2 += v * v;
  t.spec_scale = 1.0 / (16000.0 * s2);
  if ((rc = upload(&t.hamming400, ham))) return rc;
  {
    std::vector<float> hf(hann.begin(), hann.end()), tf(tuk.begin(), tuk.end()), mf(ham.begin(), ham.end());
    if ((rc = upload(&t.hann640f, hf)) || (rc = upload(&t.tukey640f, tf)) || (rc = upload(&t.hamming400f, mf)))
      return rc;
  }
  if ((rc = upload(&t.hann640, hann))) return rc;
  if ((rc = upload(&t.tukey640, tuk))) return rc;

  {
    std::vector<int4> meta;
    std::vector<float> pv;
    if ((rc = to_pairs(fbank_matrix(), 120, 257, 12, meta, pv)) || (rc = upload(&t.fbp_meta, meta)) ||
        (rc = upload(&t.fbp_w, pv)))
      return rc;
    if ((rc = upload(&t.fb_hz, fbank_hz()))) return rc;
    std::vector<int> wl;
    std::vector<float> wv;
    if ((rc = to_windows(slaney_mel(), 128, 321, 16, wl, wv)) || (rc = upload(&t.mel16_lo, wl)) ||
        (rc = upload(&t.mel16_w, wv)))
      return rc;
    std::vector<float> wt(16 * 128);
    for (int m = 0; m < 128; ++m)
      for (int q = 0; q < 16; ++q) wt[q * 128 + m] = wv[m * 16 + q];
    if ((rc = upload(&t.mel16_wt, wt))) return rc;
    // lane pairs for mfcc3_kernel.  Lane l owns one narrow filter (0..63, <= 3 bins) read as a 3-bin
    // window and one wide filter (64..127, <= 15 bins) read as a 15-bin window.  ds_read_b32 serves
    // lanes 0-31 and 32-63 as two groups over 32 banks: the narrow filters go to the groups by halves,
    // the wide ones alternately, and each wide window's start (free within [last - 14, first]) is
    // matched so that the 32 starts of a group are distinct mod 32 — every tap read conflict-free
    // (a plain lane = filter layout costs 3x on those 15 reads).
    const std::vector<double> mel = slaney_mel();
    int first[128], last[128];
    for (int m = 0; m < 128; ++m) {
      first[m] = last[m] = -1;
      for (int k = 0; k < 321; ++k)
        if (mel[(size_t)m * 321 + k] != 0.0) { if (first[m] < 0) first[m] = k; last[m] = k; }
      SRK_REQUIRE(first[m] >= 0 && last[m] - first[m] < (m < 64 ? 3 : 15), SRK_ERR_INTERNAL,
                  "mel filter %d does not fit its lane window", m);
    }
    std::vector<int4> qlo(64);
    std::vector<float> qw(18 * 64, 0.f);
    for (int g = 0; g < 2; ++g) {
      int wide[32], start[32], owner[32];
      for (int i = 0; i < 32; ++i) { wide[i] = 64 + 2 * i + g; start[i] = first[wide[i]]; }
      for (int r = 0; r < 32; ++r) owner[r] = -1;
      // Kuhn's augmenting paths: filter i -> a start s in [max(0, last - 14), min(first, 306)], residue s % 32
      std::vector<int> seen(32);
      std::function<bool(int)> assign = [&](int i) {
        const int f = wide[i];
        for (int s0 = std::max(0, last[f] - 14); s0 <= std::min(first[f], 321 - 15); ++s0) {
          const int r = s0 % 32;
          if (seen[r]) continue;
          seen[r] = 1;
          if (owner[r] < 0 || assign(owner[r])) { owner[r] = i; start[i] = s0; return true; }
        }
        return false;
      };
      bool ok = true;
      for (int i = 0; i < 32 && ok; ++i) { std::fill(seen.begin(), seen.end(), 0); ok = assign(i); }
      if (!ok)   // still correct, only slower: plain starts
        for (int i = 0; i < 32; ++i) start[i] = first[wide[i]];
      for (int i = 0; i < 32; ++i) {
        const int l = 32 * g + i, fa = 32 * g + i, fb = wide[i];
        qlo[l] = int4{first[fa], start[i], fa, fb};
        for (int q = 0; q < 3; ++q)
          if (first[fa] + q <= last[fa]) qw[q * 64 + l] = (float)mel[(size_t)fa * 321 + first[fa] + q];
        for (int q = 0; q < 15; ++q) {
          const int k = start[i] + q;
          if (k >= first[fb] && k <= last[fb]) qw[(3 + q) * 64 + l] = (float)mel[(size_t)fb * 321 + k];
        }
      }
    }
    if ((rc = upload(&t.melq_lo, qlo)) || (rc = upload(&t.melq_w, qw))) return rc;
  }

  std::vector<float> dct(13 * 128);
  for (int k = 0; k < 128; ++k) dct[k] = (float)(1.0 / std::sqrt(128.0));
  for (int i = 1; i < 13; ++i)
    for (int k = 0; k < 128; ++k)
      dct[i * 128 + k] = (float)(std::cos(i * (2 * k + 1) * M_PI / 256.0) * std::sqrt(2.0 / 128.0));
  if ((rc = upload(&t.dct, dct))) return rc;
  t.ready = true;
  return SRK_OK;
}

}  // namespace

const double* fbank_hz_points() {
  static const std::vector<double> hz = fbank_hz();
  return hz.data();
}

int get_tables(const DeviceTables** out) {
  int dev = 0;
  SRK_CHECK_HIP(hipGetDevice(&dev));
  SRK_REQUIRE(dev >= 0 && dev < kMaxDevices, SRK_ERR_INVALID, "device %d out of range", dev);
  DeviceTables& t = g_tables[dev];
  if (!t.ready) {
    std::lock_guard<std::mutex> lk(g_mutex);
    if (!t.ready) {
      int rc = build_tables(t);
      if (rc) return rc;
    }
  }
  *out = &t;
  return SRK_OK;
}

// ---------------------------------------------------------------- runtime options: the table of options.h
namespace {

// The hooked options: option_set_<hook> stores an accepted value, option_get_<hook> returns the value that sets
// the current state again.
int option_set_matmul_precision(int64_t v) { g_opt_matmul_prec.store((int)v); return SRK_OK; }
int64_t option_get_matmul_precision() { return g_opt_matmul_prec.load(); }
int option_set_gru_trace_ptr(int64_t v) { g_opt_gru_trace = reinterpret_cast<unsigned long long*>(v); return SRK_OK; }
int64_t option_get_gru_trace_ptr() { return reinterpret_cast<int64_t>(g_opt_gru_trace); }
int option_set_gru_dc_offset_ns(int64_t v) { g_opt_gru_dc_offset = (unsigned)(v / 10); return SRK_OK; }
int64_t option_get_gru_dc_offset_ns() { return (int64_t)g_opt_gru_dc_offset * 10; }
int option_set_gru_dwhh_fused(int64_t v) { g_opt_gru_dwhh_fused = (v & 1) ? (int)v : 0; return SRK_OK; }
int64_t option_get_gru_dwhh_fused() { return g_opt_gru_dwhh_fused; }
int option_set_release_scratch(int64_t) { return ScratchPool::release_all(); }
constexpr int64_t (*option_get_release_scratch)() = nullptr;

struct Accepts {
  enum Kind { kBool, kRange, kOneOf, kPointer, kAction } kind;
  int64_t lo, hi;        // kRange
  int64_t set[4]; int n;   // kOneOf
  bool ok(int64_t v) const {
    if (kind == kRange) return v >= lo && v <= hi;
    if (kind != kOneOf) return true;
    for (int i = 0; i < n; ++i)
      if (set[i] == v) return true;
    return false;
  }
  std::string text() const {
    std::string s;
    switch (kind) {
      case kBool: return "bool";
      case kRange: return std::to_string(lo) + ".." + std::to_string(hi);
      case kOneOf:
        for (int i = 0; i < n; ++i) s += (i ? "|" : "") + std::to_string(set[i]);
        return s;
      case kPointer: return "pointer";
      case kAction: return "action";
    }
    return s;
  }
};
template <class... T> constexpr int count_of(T...) { return sizeof...(T); }
#define SRK_BOOL {Accepts::kBool, 0, 0, {}, 0}
#define SRK_RANGE(lo, hi) {Accepts::kRange, lo, hi, {}, 0}
#define SRK_ONEOF(...) {Accepts::kOneOf, 0, 0, {__VA_ARGS__}, count_of(__VA_ARGS__)}
#define SRK_POINTER {Accepts::kPointer, 0, 0, {}, 0}
#define SRK_ACTION {Accepts::kAction, 0, 0, {}, 0}

struct Option {
  const char* name;
  Accepts accepts;
  int64_t def;
  const char* doc;
  int* i; unsigned* u;       // a plain option's variable (one of the two), or
  int (*set)(int64_t);       // a hooked option's store
  int64_t (*get)();          // and read (nullptr: an action)
  bool readable() const { return i || u || get; }
  int64_t value() const { return i ? *i : u ? *u : get(); }
};
inline Option plain_option(const char* name, Accepts a, int64_t def, const char* doc, int* p) {
  return {name, a, def, doc, p, nullptr, nullptr, nullptr};
}
inline Option plain_option(const char* name, Accepts a, int64_t def, const char* doc, unsigned* p) {
  return {name, a, def, doc, nullptr, p, nullptr, nullptr};
}
#define SRK_PLAIN_ENTRY(type, var, name, accepts, def, doc) plain_option(name, accepts, def, doc, &var),
#define SRK_HOOKED_ENTRY(name, hook, accepts, def, doc) \
  Option{name, accepts, def, doc, nullptr, nullptr, option_set_##hook, option_get_##hook},
const Option g_options[] = {SRK_OPTION_LIST(SRK_PLAIN_ENTRY, SRK_HOOKED_ENTRY)};

const Option* find_option(const char* name) {
  for (const Option& o : g_options)
    if (!strcmp(o.name, name)) return &o;
  return nullptr;
}

}  // namespace
}  // namespace srk

extern "C" {

int srk_version(void) { return SRK_ABI_VERSION; }

const char* srk_last_error(void) { return srk::g_last_error.c_str(); }

int srk_init(int device) {
  SRK_API_BEGIN
  int prev = 0;
  SRK_CHECK_HIP(hipGetDevice(&prev));
  SRK_CHECK_HIP(hipSetDevice(device));
  const srk::DeviceTables* t = nullptr;
  int rc = srk::get_tables(&t);
  SRK_CHECK_HIP(hipSetDevice(prev));
  return rc;
  SRK_API_END
}

int srk_set_option(const char* name, int64_t value) {
  SRK_API_BEGIN
  SRK_REQUIRE(name, SRK_ERR_INVALID, "set_option: null name");
  const srk::Option* o = srk::find_option(name);
  SRK_REQUIRE(o, SRK_ERR_INVALID, "set_option: unknown option '%s'", name);
  SRK_REQUIRE(o->accepts.ok(value), SRK_ERR_INVALID, "set_option: %s = %lld refused, it accepts %s", name,
              (long long)value, o->accepts.text().c_str());
  if (o->set) return o->set(value);
  const int64_t v = o->accepts.kind == srk::Accepts::kBool ? value != 0 : value;
  if (o->i) *o->i = (int)v; else *o->u = (unsigned)v;
  return SRK_OK;
  SRK_API_END
}

int srk_get_option(const char* name, int64_t* value) {
  SRK_API_BEGIN
  SRK_REQUIRE(name && value, SRK_ERR_INVALID, "get_option: null argument");
  const srk::Option* o = srk::find_option(name);
  SRK_REQUIRE(o, SRK_ERR_INVALID, "get_option: unknown option '%s'", name);
  SRK_REQUIRE(o->readable(), SRK_ERR_INVALID, "get_option: '%s' is an action, it has no value", name);
  *value = o->value();
  return SRK_OK;
  SRK_API_END
}

int srk_option_list(char* buf, int64_t cap, int64_t* needed) {
  SRK_API_BEGIN
  SRK_REQUIRE(needed && (buf || cap == 0), SRK_ERR_INVALID, "option_list: null pointer");
  std::string out;
  for (const srk::Option& o : srk::g_options) {
    const bool action = !o.readable();   // no default and no value: both columns say "action"
    out += std::string(o.name) + "\t" + (action ? "action" : std::to_string(o.def)) + "\t" +
           (action ? "action" : std::to_string(o.value())) + "\t" + o.accepts.text() + "\t" + o.doc + "\n";
  }
  *needed = (int64_t)out.size() + 1;
  if (cap > 0) {
    const size_t n = std::min<size_t>(out.size(), (size_t)cap - 1);
    memcpy(buf, out.data(), n);
    buf[n] = 0;
  }
  return SRK_OK;
  SRK_API_END
}

}  // extern "C"

extern "C" int64_t srk_scratch_generation(void) { return srk::g_scratch_gen.load(); }
