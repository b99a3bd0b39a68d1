// Host build of layout_dm_amd/csrc/ldm_refine_core.h (the arithmetic of kernels_refine.hip), laid out like the kernel: one
// "workgroup" per (layout, chunk), its tokens staged and range-checked first (or read in place beyond kMaxStaged), then
// every thread's groups of four floats.  tests/test_refine_prior.py runs it against layoutdm.refinement_weak_logits, and once
// more built with -fsanitize=address,undefined: the token array, the table and the END of the output are exact-size
// allocations, so a read or write past them stops the run.
//
// in:  int32 {seq_i64, B_seq, B, S, C, mis}, float32 weight, tokens [B_seq][S] (int64 if seq_i64 else int32), table float32 [C][C]
//      mis = 0..3: floats the output starts past a 16-byte boundary (what a slice of a larger buffer gives the kernel)
// out: int32 error word (bit 0 = a token outside [0, C)), then float32 [B][C][S]
// exit 2: malformed input or refused arguments; 3: a float in front of the output was touched; 4: a float of it was not written
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_refine_core.h"
#include "cpu_check_io.h"

namespace {

namespace R = ldm_refine;

constexpr uint32_t kSentinel = 0x7fc0dead;  // a NaN no product of the table is

struct StagedTokens {
  const int32_t* toks;
  int32_t operator()(int s) const { return toks[s]; }
};

struct DirectTokens {
  const void* seq;
  int seq_i64, C;
  int64_t row_off;
  int32_t* err;
  int32_t operator()(int s) const {
    const int32_t t = R::checked_token(R::load_token(seq, seq_i64, row_off + s), C);
    if (t < 0) *err = R::kErrToken;
    return t;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* f = check_io::open_or_exit(argv[1], "rb", 1);
  int32_t hdr[6];
  float weight;
  if (fread(hdr, 4, 6, f) != 6 || fread(&weight, 4, 1, f) != 1) return 2;
  const int seq_i64 = hdr[0], B_seq = hdr[1], B = hdr[2], S = hdr[3], C = hdr[4], mis = hdr[5];
  if (!R::args_ok(seq_i64, B_seq, B, S, C) || mis < 0 || mis >= R::kVec) return 2;
  const size_t n_tok = (size_t)B_seq * S, tok_bytes = n_tok * (seq_i64 ? 8 : 4);
  void* seq = malloc(tok_bytes ? tok_bytes : 1);   // exact size: the sanitizer sees a read past the last token
  float* table = static_cast<float*>(malloc((size_t)C * C * 4));
  if (!seq || !table || fread(seq, 1, tok_bytes, f) != tok_bytes || fread(table, 4, (size_t)C * C, f) != (size_t)C * C) return 2;
  fclose(f);

  const int64_t CS = R::slab_size(S, C);
  const size_t n_out = (size_t)B * (size_t)CS;
  void* raw = nullptr;
  if (posix_memalign(&raw, 16, (mis + n_out) * 4 + (mis + n_out == 0 ? 16 : 0)) != 0) return 1;
  uint32_t* bits = static_cast<uint32_t*>(raw);
  for (size_t i = 0; i < mis + n_out; ++i) bits[i] = kSentinel;
  float* out = static_cast<float*>(raw) + mis;
  int32_t err = 0;
  if (B > 0) {
    if (R::misalign_of(out) != mis) return 1;
    const int64_t n_chunk = R::chunks_per_layout(S, C);
    std::vector<int32_t> lds(S <= R::kMaxStaged ? S : 0);
    for (int64_t b = 0; b < B; ++b)
      for (int64_t k = 0; k < n_chunk; ++k) {
        if (!R::chunk_live(k, b, mis, S, C)) continue;
        const int64_t row_off = R::seq_row(b, B_seq) * S;
        float* slab = out + b * CS;
        if (S <= R::kMaxStaged) {
          for (int s = 0; s < S; ++s) {
            lds[s] = R::checked_token(R::load_token(seq, seq_i64, row_off + s), C);
            if (lds[s] < 0) err = R::kErrToken;
          }
          for (int tid = 0; tid < R::kBlock; ++tid)
            R::thread_work(tid, k, b, mis, S, C, table, weight, slab, StagedTokens{lds.data()});
        } else {
          for (int tid = 0; tid < R::kBlock; ++tid)
            R::thread_work(tid, k, b, mis, S, C, table, weight, slab, DirectTokens{seq, seq_i64, C, row_off, &err});
        }
      }
  }
  for (int i = 0; i < mis; ++i)
    if (bits[i] != kSentinel) return 3;
  for (size_t i = 0; i < n_out; ++i)
    if (bits[mis + i] == kSentinel) return 4;
  f = check_io::open_or_exit(argv[2], "wb", 1);
  check_io::write_vec(f, &err, 1);
  check_io::write_vec(f, out, n_out);
  fclose(f);
  free(raw), free(table), free(seq);
  return 0;
}
