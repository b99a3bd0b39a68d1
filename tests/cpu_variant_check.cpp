// Host check of layout_dm_amd/csrc/ldm_variant_core.h — the load-time arithmetic of the denoiser variants, the same source the device
// compiles (kernels_norm.hip sinus_table_k / adaln_const_table_k) — built with plain g++ (and as the ASan + UBSan build) and run as its own
// process by tests/test_denoiser_variants.py.
//   sinus T D out.bin          the [T][D] float32 table of timestep_type *_abs, entry by entry as the kernel's threads write it
//   const D in.bin out.bin     in: nn.LayerNorm's weight [D] | bias [D] (float32); out: the [2 D] AdaLN row of timestep_type None
// Exit codes: 0, 2 usage / bad arguments, 3 input file, 4 output file.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_variant_core.h"
#include "cpu_check_io.h"

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "sinus")) {
    const int T = atoi(argv[2]), D = atoi(argv[3]);
    if (!ldm_variant::sinusoid_args_ok(T, D) || T > 100000 || D > 4096) return 2;
    const int half = D / 2;
    std::vector<float> out((size_t)T * D);
    for (int i = 0; i < T * half; ++i) {   // (the kernel's thread index)
      const int t = i / half, k = i % half;
      ldm_variant::sinusoid_pair(t, T, k, half, &out[(size_t)t * D + k], &out[(size_t)t * D + half + k]);
    }
    FILE* f = check_io::open_or_exit(argv[4], "wb", 4);
    const bool ok = check_io::write_vec(f, out);
    fclose(f);
    return ok ? 0 : 4;
  }
  if (argc == 5 && !strcmp(argv[1], "const")) {
    const int D = atoi(argv[2]);
    if (D < 1 || D > 4096) return 2;
    FILE* f = check_io::open_or_exit(argv[3], "rb", 3);
    std::vector<float> in;
    const bool read = check_io::read_vec(f, in, (size_t)2 * D);
    fclose(f);
    if (!read) return 3;
    std::vector<float> out((size_t)2 * D);
    for (int j = 0; j < 2 * D; ++j) out[j] = ldm_variant::const_row_entry(in.data(), in.data() + D, D, j);
    f = check_io::open_or_exit(argv[4], "wb", 4);
    const bool ok = check_io::write_vec(f, out);
    fclose(f);
    return ok ? 0 : 4;
  }
  return 2;
}
