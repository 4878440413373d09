// gamma_monotone.cpp -- one-off check behind the device's RGB8 table (common/gamma_table.h).
//
// The table of 255 thresholds reproduces the host's byte nearbyint(min(1, max(0, powf(v, 1/2.2f))) * 255)
// for every v only if that byte never decreases as v grows.  This program walks every binary32 of
// [+0, 1] in order, reports every inversion, and then compares the table lookup (count of t[k] <= v)
// with the expression at every one of those values.  Exit status 0: monotone and equal everywhere.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -o build/gamma_monotone tools/gamma_monotone.cpp
//   build/gamma_monotone
#include <cstdio>

#include "../bling_amd/csrc/common/gamma_table.h"

int main() {
  float t[255];
  bgamma::thresholds(t);
  unsigned long long inversions = 0, mismatches = 0, walked = 0;
  int prev = 0, k = 0;   // k = thresholds already passed = the table's byte
  for (uint32_t b = 0; b <= 0x3F800000u; ++b) {
    const float v = bgamma::from_bits(b);
    const int byte = bgamma::host_byte(v);
    if (byte < prev) {
      if (inversions++ < 16) std::printf("inversion at bits 0x%08x (%.9g): byte %d after %d\n", b, v, byte, prev);
    }
    prev = byte;
    while (k < 255 && t[k] <= v) ++k;
    if (k != byte && mismatches++ < 16) std::printf("table mismatch at bits 0x%08x (%.9g): table %d, host %d\n", b, v, k, byte);
    ++walked;
  }
  std::printf("walked %llu binary32 values of [0, 1]: %llu inversions, %llu table mismatches; t[0] = %.9g, t[254] = %.9g\n",
              walked, inversions, mismatches, t[0], t[254]);
  return inversions == 0 && mismatches == 0 ? 0 : 1;
}
