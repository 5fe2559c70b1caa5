// env_accel_checker.cpp — TEST INFRASTRUCTURE: the environment's importance table (include/rt_abi.h "The environment") restated on the CPU with
// sequential loops and unsigned __int128, sharing no code with csrc/env_accel.h.  Where the product binary-searches two prefix arrays, this file walks the smalls
// and the larges once, Vose-style, with the deficits handed out and the excesses reached as two running 128-bit sums, and divides with the compiler's 128-bit division; where the product shifts a float's bits, this file calls
// frexp / ldexp / rint.  tests/env.py drives it through ctypes; tests/env_san_main.cpp links it into a program of its own.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

typedef unsigned __int128 u128;

struct Entry { int32_t alias; float q, pdf, aliasPdf; };

struct Prepared {
  std::vector<float> imp, mx, lum;
  bool refused = false;
};

bool posInf(float v) { return std::isinf(v) && v > 0; }

Prepared prepare(int w, int h, const float* px)
{
  Prepared p;
  const uint32_t rx = uint32_t(w), ry = uint32_t(h);
  p.imp.resize(size_t(rx) * ry); p.mx.resize(p.imp.size()); p.lum.resize(p.imp.size());
  float cosTheta0 = 1.0f;
  const float stepPhi = float(2.0 * M_PI) / float(rx);
  const float stepTheta = float(M_PI) / float(ry);
  for(uint32_t y = 0; y < ry; ++y) {
    const float cosTheta1 = std::cos(float(y + 1) * stepTheta);
    const float area = (cosTheta0 - cosTheta1) * stepPhi;
    cosTheta0 = cosTheta1;
    for(uint32_t x = 0; x < rx; ++x) {
      const size_t i = size_t(y) * rx + x;
      const float r = px[i * 4], g = px[i * 4 + 1], b = px[i * 4 + 2];
      const float mx = std::max(r, std::max(g, b));
      float imp = area * mx;
      if(!(mx > 0.0f) || !(imp > 0.0f)) imp = 0.0f;
      float lum = r * 0.2126f + g * 0.7152f + b * 0.0722f;
      if(!(lum > 0.0f)) lum = 0.0f;
      p.imp[i] = imp; p.mx[i] = mx > 0.0f ? mx : 0.0f; p.lum[i] = lum;
      if(posInf(r) || posInf(g) || posInf(b) || posInf(imp) || posInf(lum)) p.refused = true;
    }
  }
  return p;
}

// the e with M 2^e in [2^39, 2^40); any e for M == 0 (every weight is then 0)
int scaleExp(float M)
{
  if(!(M > 0.0f)) return 0;
  int x = 0;
  (void)std::frexp(double(M), &x);   // M = f 2^x, f in [0.5, 1)
  return 40 - x;
}
// sum of the values quantised against their maximum; W (optional) takes the weights
uint64_t quantisedSum(const std::vector<float>& v, int& e, std::vector<uint64_t>* W)
{
  float M = 0.0f;
  for(float x : v) M = std::max(M, x);
  e = scaleExp(M);
  uint64_t T = 0;
  if(W) W->assign(v.size(), 0);
  for(size_t i = 0; i < v.size(); i++) {
    const uint64_t w = uint64_t(std::rint(std::ldexp(double(v[i]), e)));   // round to nearest even (the default rounding mode)
    if(W) (*W)[i] = w;
    T += w;
  }
  return T;
}

}  // namespace

extern "C" {

// the quantised weights and their sum (the distribution the table must reproduce): 0, or 1 when the map is refused
int evc_weights(int w, int h, const float* px, uint64_t* W, uint64_t* T)
{
  const Prepared p = prepare(w, h, px);
  if(p.refused) return 1;
  int e;
  std::vector<uint64_t> Wv;
  *T = quantisedSum(p.imp, e, &Wv);
  std::memcpy(W, Wv.data(), Wv.size() * 8);
  return 0;
}

void evc_importance(int w, int h, const float* px, float* out)
{
  const Prepared p = prepare(w, h, px);
  std::memcpy(out, p.imp.data(), p.imp.size() * 4);
}

// the whole table: 0, or 1 when the map is refused (nothing written)
int evc_accel(int w, int h, const float* px, Entry* out, float* integral, float* average, uint32_t* numSmall)
{
  const Prepared p = prepare(w, h, px);
  if(p.refused) return 1;
  const uint32_t n = uint32_t(w) * uint32_t(h);
  int e, eL;
  std::vector<uint64_t> W;
  const uint64_t T = quantisedSum(p.imp, e, &W);
  const uint64_t TL = quantisedSum(p.lum, eL, nullptr);
  *integral = float(std::ldexp(double(T), -e));
  *average = float(std::ldexp(double(TL), -eL) / double(n));
  std::vector<uint32_t> smalls, larges;
  for(uint32_t i = 0; i < n; i++) (u128(n) * W[i] < u128(T) ? smalls : larges).push_back(i);
  *numSmall = uint32_t(smalls.size());
  for(uint32_t i = 0; i < n; i++) { out[i].alias = int32_t(i); out[i].q = 1.0f; }
  if(!smalls.empty()) {
    // q lives on the grid of 2^-24 steps: a cumulative deficit or excess X is marked at (X 2^24 + T / 2) / T, and what a texel gives away is the difference
    // of two marks, so the shares that one large collects from any number of smalls add up to a difference of two marks as well
    auto mark = [&](u128 X) { return uint64_t(((X << 24) + u128(T >> 1)) / u128(T)); };
    auto keep = [&](uint64_t steps) { return float(std::ldexp(double((uint64_t(1) << 24) - steps), -24)); };
    size_t j = 0;
    u128 given = 0;                                        // the deficits handed out so far
    u128 have = u128(n) * W[larges[0]] - u128(T);          // the excesses of the larges up to the current one
    auto exhaust = [&] {   // the last small overdrew the current large: it keeps its bucket less the overdraft and takes that from the next large, which inherits the debt
      out[larges[j]].q = keep(mark(given) - mark(have));
      out[larges[j]].alias = int32_t(larges[j + 1]);
      j++;
      have += u128(n) * W[larges[j]] - u128(T);
    };
    for(uint32_t k : smalls) {
      while(have < given && j + 1 < larges.size()) exhaust();   // (a next large exists whenever the current one is overdrawn: sum of the deficits = sum of the excesses)
      const u128 before = given;
      given += u128(T) - u128(n) * W[k];
      out[k].alias = int32_t(larges[j]);
      out[k].q = keep(mark(given) - mark(before));
    }
    while(have < given && j + 1 < larges.size()) exhaust();
  }
  const float inv = *integral > 0.0f ? 1.0f / *integral : 0.0f;
  for(uint32_t i = 0; i < n; i++) out[i].pdf = *integral > 0.0f ? p.mx[i] * inv : 0.0f;
  for(uint32_t i = 0; i < n; i++) out[i].aliasPdf = out[size_t(out[i].alias)].pdf;
  return 0;
}

}  // extern "C"
