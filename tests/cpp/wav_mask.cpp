// wav_probe's view of a RIFF/WAVE header (needle_amd/csrc/hostutil.cpp), for tests/test_channel_mix_cpu.py: prints
// "<channels> <sample rate> <bits> <channel mask in hex>" of every file named, or "error" where the probe refuses it.
#include <cstdio>

#include "common.h"

int main(int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    needle::WavInfo info;
    if (needle::wav_probe(argv[i], &info).ok()) std::printf("%d %d %d 0x%X\n", info.channels, info.sample_rate, info.bits, info.channel_mask);
    else std::printf("error\n");
  }
  return 0;
}
