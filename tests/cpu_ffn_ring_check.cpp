// CPU replay of the LDS map of FfnStream's two-stage ring (layout_dm_amd/csrc/ldm_stream_sched.h: FfnRingLinear — the
// hybrid kernel's — and FfnRingInterleaved — the stack kernel's): what the 4 x 16 LDS-DMA pieces of a stage write against
// what the fragment reads of the stream fetch, byte by byte.  No HIP, no GPU.
//
//   * both stages are inside the 128-KiB ring, disjoint, and the DMA of a stage writes each of its 64 KiB exactly once;
//   * every fragment read (29 W1 items + 30 W2 items, 64 lanes x 16 bytes; the four waves read the same addresses) hits
//     bytes the DMA of THAT stage wrote, no two reads of a stage overlap, and the sequence of IMAGE bytes read is the
//     same for both maps and both stages: 59 x 1 KiB distinct bytes (the rest of a stage's 64 KiB is the image's padding
//     — K 464 -> 512, 30 of 32 W2 KiB — which the DMA writes and nothing reads);
//   * every immediate of the interleaved map fits the 16-bit offset field of ds_read, for either stage;
//   * the interleaved map is a bijection of the linear one: the same (item, lane, byte) reads the same IMAGE byte, and
//     the same (wave, piece, lane, byte) of the DMA carries the same image byte.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_stream_sched.h"

namespace {

constexpr int KS = 29, NT2 = 15, NIT = KS + 1 + 2 * NT2, NW = 4, NPIECE = 16, NLANE = 64;
constexpr unsigned kRing = 0x20000u, kStageBytes = 0x10000u;

int fails = 0;
#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c)) {                            \
      if (++fails < 20) {                  \
        std::printf("FAIL %s: ", #c);      \
        std::printf(__VA_ARGS__);          \
        std::printf("\n");                 \
      }                                    \
    }                                      \
  } while (0)

// LDS byte -> image byte of the stage the DMA pieces carry there (-1: not written)
template <class MAP>
std::vector<int> dma_image(int s) {
  std::vector<int> lds(kRing, -1);
  for (int w = 0; w < NW; ++w)
    for (int k = 0; k < NPIECE; ++k)
      for (int lane = 0; lane < NLANE; ++lane)
        for (int b = 0; b < 16; ++b) {
          const unsigned dst = MAP::dma_dst(s, w, k) + lane * 16 + b;  // one global_load_lds_dwordx4: 64 lanes x 16 bytes = 1 KiB
          const int img = w * 16384 + k * 1024 + lane * 16 + b;
          CHECK(dst < kRing, "stage %d wave %d piece %d: LDS byte %u outside the ring", s, w, k, dst);
          if (dst >= kRing) continue;
          CHECK(lds[dst] < 0, "stage %d: LDS byte %u written twice", s, dst);
          lds[dst] = img;
        }
  return lds;
}

// the LDS byte address of byte b of lane `lane`'s read of queue item I of a chunk in stage s
template <class MAP>
unsigned read_addr(int I, int s, int lane, int b) {
  const int r = lane & 31, hi = lane >> 5;
  const unsigned reg = MAP::template reg_base<KS, NT2>(I) +
                       (I < KS ? ldm_sched::ffn_w1_lane(r, hi, I & 7) : ldm_sched::ffn_w2_lane(r, hi, (I - KS - 1) / NT2));
  return reg + MAP::template imm<KS, NT2>(I, s) + b;
}

// image bytes read by (item, lane, byte), in that order
template <class MAP>
std::vector<int> read_image(int s, const std::vector<int>& lds) {
  std::vector<int> out;
  std::set<unsigned> seen;
  for (int I = 0; I < NIT; ++I) {
    if (I == KS) continue;  // the pseudo item's data is never used (it re-reads W1 column 0)
    for (int lane = 0; lane < NLANE; ++lane)
      for (int b = 0; b < 16; ++b) {
        const unsigned a = read_addr<MAP>(I, s, lane, b);
        CHECK(a < kRing, "item %d stage %d lane %d: LDS byte %u outside the ring", I, s, lane, a);
        if (a >= kRing) {
          out.push_back(-2);
          continue;
        }
        CHECK(lds[a] >= 0, "item %d stage %d lane %d: LDS byte %u not written by this stage's DMA", I, s, lane, a);
        CHECK(seen.insert(a).second, "item %d stage %d lane %d: LDS byte %u read twice", I, s, lane, a);
        out.push_back(lds[a]);
      }
  }
  return out;
}

}  // namespace

int main() {
  using LIN = ldm_sched::FfnRingLinear;
  using ILV = ldm_sched::FfnRingInterleaved;
  std::vector<int> lin[2] = {dma_image<LIN>(0), dma_image<LIN>(1)};
  std::vector<int> ilv[2] = {dma_image<ILV>(0), dma_image<ILV>(1)};
  // stages: disjoint, 64 KiB each, together the ring
  for (auto* m : {lin, ilv}) {
    unsigned n0 = 0, n1 = 0;
    for (unsigned a = 0; a < kRing; ++a) {
      CHECK(!(m[0][a] >= 0 && m[1][a] >= 0), "LDS byte %u belongs to both stages", a);
      n0 += m[0][a] >= 0;
      n1 += m[1][a] >= 0;
    }
    CHECK(n0 == kStageBytes && n1 == kStageBytes, "stage sizes %u %u", n0, n1);
  }
  // the halves lie where the map says: W1 tile = image [0, 32 KiB), W2 slab = image [32 KiB, 64 KiB)
  for (int s = 0; s < 2; ++s)
    for (unsigned o = 0; o < 0x8000u; ++o) {
      CHECK(ilv[s][ILV::w1(s) + o] == (int)o, "interleaved W1 stage %d offset %u", s, o);
      CHECK(ilv[s][ILV::w2(s) + o] == (int)(0x8000u + o), "interleaved W2 stage %d offset %u", s, o);
      CHECK(lin[s][LIN::w1(s) + o] == (int)o, "linear W1 stage %d offset %u", s, o);
      CHECK(lin[s][LIN::w2(s) + o] == (int)(0x8000u + o), "linear W2 stage %d offset %u", s, o);
    }
  // immediates: both stages of the interleaved map within the offset field; the linear map's stage 1 is not (that is
  // why it toggles its registers)
  for (int I = 0; I < NIT; ++I) {
    for (int s = 0; s < 2; ++s) {
      const unsigned im = ILV::imm<KS, NT2>(I, s);
      CHECK(im < 65536u, "item %d stage %d immediate %u", I, s, im);
    }
    const unsigned l0 = LIN::imm<KS, NT2>(I, 0), l1 = LIN::imm<KS, NT2>(I, 1);
    CHECK(l0 < 65536u && l1 >= 65536u, "linear item %d: %u %u", I, l0, l1);
  }
  // reads: inside the stage's DMA, no overlap, and the same image bytes whatever the map and the stage
  const std::vector<int> ref = read_image<LIN>(0, lin[0]);
  CHECK(ref.size() == (size_t)(NIT - 1) * NLANE * 16, "%zu bytes read", ref.size());
  {
    std::set<int> distinct(ref.begin(), ref.end());
    CHECK(distinct.size() == ref.size(), "%zu distinct image bytes for %zu read", distinct.size(), ref.size());
  }
  CHECK(read_image<LIN>(1, lin[1]) == ref, "linear stage 1 reads other image bytes than stage 0");
  for (int s = 0; s < 2; ++s) CHECK(read_image<ILV>(s, ilv[s]) == ref, "interleaved stage %d reads other image bytes than the linear map", s);
  // bijection of the maps: LDS byte of the linear stage -> image byte -> LDS byte of the interleaved stage, both ways
  for (int s = 0; s < 2; ++s) {
    std::vector<int> where(kStageBytes, -1);
    for (unsigned a = 0; a < kRing; ++a)
      if (ilv[s][a] >= 0) {
        CHECK(where[ilv[s][a]] < 0, "image byte %d twice in interleaved stage %d", ilv[s][a], s);
        where[ilv[s][a]] = (int)a;
      }
    for (unsigned a = 0; a < kRing; ++a)
      if (lin[s][a] >= 0) CHECK(where[lin[s][a]] >= 0, "image byte %d of linear stage %d has no place in the interleaved one", lin[s][a], s);
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("OK: FFN ring maps: 2 stages x 64 DMA pieces, %d fragment items x 64 lanes, immediates < 65536, linear <-> interleaved bijective\n", NIT - 1);
  return 0;
}
