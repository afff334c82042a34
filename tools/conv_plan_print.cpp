// Prints the conv plan (csrc/conv_plan.cpp) of the benchmark's four single-GPU configurations under the default options:
// per layer and pass the kernel form, and for the F(4x4,3x3) forward / data-gradient launches the block shape.  Needs no
// device.  A stand-alone program, so that the planner's host code can run under the sanitizers:
//
//   cd image-generation_amd && make
//   hipcc -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -c csrc/conv_plan.cpp -o /tmp/conv_plan.san.o
//   hipcc -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -c ../tools/conv_plan_print.cpp -o /tmp/conv_plan_print.san.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/conv_plan_print /tmp/conv_plan_print.san.o \
//       /tmp/conv_plan.san.o $(ls build/*.o | grep -v conv_plan.cpp.o)
//   /tmp/conv_plan_print
#include <cstdio>

#include "../image-generation_amd/csrc/conv_plan.h"

using namespace dvg;

static const char* kForm[CF_COUNT] = {"direct", "fold", "d22", "lc0", "wino2", "wino4"};

static void print_layer(const char* net, int l, const ConvLayer& c) {
  std::printf("  %s layer %d  M=%-8lld %4d -> %-4d side %-2d  fwd %-6s%s  dgrad %-6s%s  wgrad %s\n", net, l, (long long)c.M, c.Cin,
              c.Cout, 1 << c.L, kForm[c.form[PASS_FWD]], c.form[PASS_FWD] == CF_WINO4 ? (c.block64[PASS_FWD] ? " 32x64" : " 64x32") : "",
              kForm[c.form[PASS_DGRAD]], c.form[PASS_DGRAD] == CF_WINO4 ? (c.block64[PASS_DGRAD] ? " 32x64" : " 64x32") : "",
              kForm[c.form[PASS_WGRAD]]);
}

int main() {
  struct Cfg { const char* name; int64_t B; int n, R; };
  const Cfg cfgs[4] = {{"c3", 4096, 512, 8}, {"c2", 256, 128, 8}, {"c1", 64, 64, 8}, {"c5", 256, 1024, 8}};  // (bench.py: CONFIGS)
  const PlanOptions o = plan_options();
  for (const Cfg& c : cfgs) {
    std::printf("%s: B = %lld, n = %d, %d replicas\n", c.name, (long long)c.B, c.n, c.R);
    ConvLayer e[4], d[3];
    plan_encoder_layers(c.B, c.n, true, o, e);
    for (int l = 1; l < 4; ++l) print_layer("encoder", l, e[l]);
    plan_decoder_layers(c.B * c.R, c.n, o, d);
    for (int l = 0; l < 3; ++l) print_layer("decoder", l, d[l]);
  }
  return 0;
}
