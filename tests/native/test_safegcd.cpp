// Host check of zk_inv.hpp (the device inversion's code, compiled for the CPU): prints
// "<field> <x> <x^-1>" lines in hex for tests/test_native.py to verify with Python big integers.
// Lines "<field> <x>" (hex, below the modulus) on stdin are appended to the inputs of both limb
// forms of that field: the edge values of tests/field_edges.py.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <map>
#include <random>
#include <string>
#include <vector>
#include "zk_inv.hpp"
#include "zk_params.inc"

struct Words { uint64_t w[6]; };
static std::map<std::string, std::vector<Words>> extra;  // per field, from stdin

static void read_extra() {
  char name[64], hex[128];
  while (scanf("%63s %127s", name, hex) == 2) {
    Words v = {{0, 0, 0, 0, 0, 0}};
    const int len = (int)strlen(hex);
    for (int i = 0; i < len; i++) {  // hex digit i counts from the least significant end
      const char ch = hex[len - 1 - i];
      const uint64_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
      if (i < 96) v.w[i / 16] |= d << (4 * (i % 16));
    }
    extra[name].push_back(v);
  }
}

template <int L, int NB, int B = 62>
static void run(const char *name, const int64_t (&P)[L], uint64_t pinv, int n64, const uint64_t *pw, int count,
                std::mt19937_64 &rng) {
  const std::vector<Words> &ex = extra[name];
  for (int k = 0; k < count + (int)ex.size(); k++) {
    uint64_t x[6] = {0, 0, 0, 0, 0, 0}, y[6];
    if (k >= count) {
      for (int i = 0; i < n64; i++) x[i] = ex[k - count].w[i];
    } else if (k == 0) x[0] = 1;
    else if (k == 1) {  // p - 1
      for (int i = 0; i < n64; i++) x[i] = pw[i];
      x[0] -= 1;
    } else if (k == 2) x[0] = 2;
    else if (k == 3) x[0] = 0;  // 0 -> 0
    else {
      for (int i = 0; i < n64; i++) x[i] = rng();
      // reduce below p by clearing the top bits beyond p's top word and subtracting p while >= p
      int top = 63;
      while (!((pw[n64 - 1] >> top) & 1)) top--;
      x[n64 - 1] &= (top == 63) ? ~0ull : ((1ull << (top + 1)) - 1);
      for (;;) {
        int ge = 1;
        for (int i = n64 - 1; i >= 0; i--) {
          if (x[i] != pw[i]) { ge = x[i] > pw[i]; break; }
        }
        if (!ge) break;
        uint64_t br = 0;
        for (int i = 0; i < n64; i++) {
          const uint64_t a = x[i], b = pw[i] + br;
          br = (b < br) || (a < b);
          x[i] = a - b;
        }
      }
    }
    zk::sg_inverse_words<L, NB, B>(y, x, n64, P, pinv);
    printf("%s ", name);
    for (int i = n64 - 1; i >= 0; i--) printf("%016llx", (unsigned long long)x[i]);
    printf(" ");
    for (int i = n64 - 1; i >= 0; i--) printf("%016llx", (unsigned long long)y[i]);
    printf("\n");
  }
}

// Bernstein-Yang (safegcd, Theorem 11.2): ceil((49 d + 57) / 17) divsteps invert every input below a
// d-bit modulus (d >= 46).  Each limb layout must run at least that many: batches x steps per batch.
constexpr int divstep_bound(int d) { return (49 * d + 57 + 16) / 17; }
#define CHECK_DIVSTEPS(FIELD, BITS)                                                                      \
  static_assert(FIELD##_S62_BATCHES * 62 >= divstep_bound(BITS), #FIELD ": too few 62-step batches");   \
  static_assert(FIELD##_S60_BATCHES * 60 >= divstep_bound(BITS), #FIELD ": too few 60-step batches")
static_assert(divstep_bound(381) == 1102 && divstep_bound(255) == 739 && divstep_bound(254) == 736, "bound");
CHECK_DIVSTEPS(ZK_BLS12_381_FP, 381);  // 60-step layout: 19 x 60 = 1140 >= 1102
CHECK_DIVSTEPS(ZK_BLS12_381_FR, 255);  // 13 x 60 = 780 >= 739
CHECK_DIVSTEPS(ZK_BN128_FP, 254);
CHECK_DIVSTEPS(ZK_BN128_FR, 254);

int main() {
  read_extra();
  std::mt19937_64 rng(12345);
  {
    static const int64_t P[] = ZK_BLS12_381_FP_S62_P;
    const uint64_t pw[6] = {0xb9feffffffffaaabull, 0x1eabfffeb153ffffull, 0x6730d2a0f6b0f624ull,
                            0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull, 0x1a0111ea397fe69aull};
    static const int64_t P60[] = ZK_BLS12_381_FP_S60_P;
    run<ZK_BLS12_381_FP_S60_L, ZK_BLS12_381_FP_S60_BATCHES, 60>("bls12_381_fp", P60, ZK_BLS12_381_FP_S62_PINV, 6, pw, 1000, rng);
    run<ZK_BLS12_381_FP_S62_L, ZK_BLS12_381_FP_S62_BATCHES>("bls12_381_fp", P, ZK_BLS12_381_FP_S62_PINV, 6, pw,
                                                            2000, rng);
  }
  {
    static const int64_t P[] = ZK_BLS12_381_FR_S62_P;
    const uint64_t pw[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull,
                            0x73eda753299d7d48ull};
    static const int64_t P60[] = ZK_BLS12_381_FR_S60_P;
    run<ZK_BLS12_381_FR_S60_L, ZK_BLS12_381_FR_S60_BATCHES, 60>("bls12_381_fr", P60, ZK_BLS12_381_FR_S62_PINV, 4, pw, 1000, rng);
    run<ZK_BLS12_381_FR_S62_L, ZK_BLS12_381_FR_S62_BATCHES>("bls12_381_fr", P, ZK_BLS12_381_FR_S62_PINV, 4, pw,
                                                            2000, rng);
  }
  {
    static const int64_t P[] = ZK_BN128_FP_S62_P;
    const uint64_t pw[4] = {0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull,
                            0x30644e72e131a029ull};
    static const int64_t P60[] = ZK_BN128_FP_S60_P;
    run<ZK_BN128_FP_S60_L, ZK_BN128_FP_S60_BATCHES, 60>("bn128_fp", P60, ZK_BN128_FP_S62_PINV, 4, pw, 1000, rng);
    run<ZK_BN128_FP_S62_L, ZK_BN128_FP_S62_BATCHES>("bn128_fp", P, ZK_BN128_FP_S62_PINV, 4, pw, 2000, rng);
  }
  {
    static const int64_t P[] = ZK_BN128_FR_S62_P;
    const uint64_t pw[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull,
                            0x30644e72e131a029ull};
    static const int64_t P60[] = ZK_BN128_FR_S60_P;
    run<ZK_BN128_FR_S60_L, ZK_BN128_FR_S60_BATCHES, 60>("bn128_fr", P60, ZK_BN128_FR_S62_PINV, 4, pw, 1000, rng);
    run<ZK_BN128_FR_S62_L, ZK_BN128_FR_S62_BATCHES>("bn128_fr", P, ZK_BN128_FR_S62_PINV, 4, pw, 2000, rng);
  }
  return 0;
}
