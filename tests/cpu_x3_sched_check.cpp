// Host dump of layout_dm_amd/csrc/ldm_x3_sched.h — the header kernels_lngemm.hip and kernels_attnout.hip compile — as tables of
// "key=value" lines, one per step / lane / head.  Built with plain g++ and run as its own process by tests/_x3_sched.py; the replays of
// tests/test_lngemm_sched.py and tests/test_attnout_layout.py and the ISA tie of tests/test_kernel_asm_lint.py read these tables, so
// what they check is what the kernels compiled.  The header's static_asserts are checked by compiling this file.
#include <cstdio>
#include <cstdlib>

#include "../layout_dm_amd/csrc/ldm_x3_sched.h"

using namespace ldm_sched;

#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fprintf(stderr, "\n");          \
      exit(1);                        \
    }                                 \
  } while (0)

// the tile loop (lg_step), NP products per k16-step
static void dump_lg(int NP) {
  using S = LgSched;
  for (int it = 0; it < S::NIT; ++it) {
    const int ri = S::read_item(it);
    printf("lg np=%d it=%d real=%d wait=%d rpi=%d piece=%d dma=%d doff=%d begin=%d adv=%d ri=%d read=%d behind=%d roff=%d rcol=%d flip=%d sync=%d "
           "slice=%d epi=%d drain=%d writes=%d\n",
           NP, it, it < S::KS, it < S::KS ? S::wait(it, NP) : -1, S::rpi(NP), S::piece(it), S::has_dma(it, NP), S::dma_off(it, NP), S::dma_begin(it, NP),
           S::dma_advance(it, NP), ri, S::reads(it), S::reads_behind_barrier(it), S::read_off(ri), S::read_col(ri), it == S::FLIP, it == S::SYNC,
           S::slice_step(it), S::epi_lds_ops(it), it == S::KS ? S::EPI_DRAIN : -1, it == S::KS ? S::EPI_WRITES : 0);
  }
}

// the GEMM prologue (lp_step)
static void dump_lp(int NP) {
  using S = LpSched;
  for (int it = 0; it < S::NIT; ++it) {
    const int ri = S::read_item(it);
    printf("lp np=%d it=%d real=1 wait=%d rpi=%d piece=%d dma=%d doff=%d begin=%d adv=%d ri=%d read=%d behind=%d roff=%d rreg=%d flip=%d sync=%d "
           "aload=%d a_loads=%d\n",
           NP, it, S::wait(NP), S::rpi(NP), S::piece(it), S::has_dma(it, NP), S::dma_off(it, NP), S::dma_begin(it, NP), S::dma_advance(it, NP), ri,
           S::reads(it), it == S::SYNC, S::read_off(ri), S::read_reg(ri), it == S::FLIP, it == S::SYNC, it == S::A_STEP, S::a_loads(NP));
  }
}

int main() {
  printf("lg_const KS=%d NIT=%d PF=%d SYNC=%d first_group=%d\n", LgSched::KS, LgSched::NIT, LgSched::PF, LgSched::SYNC, LgSched::first_group());
  for (int np = 3; np >= 1; --np) dump_lg(np);
  printf("lp_const KS=%d NIT=%d PF=%d SYNC=%d first_group=%d NT=%d A_STEP=%d\n", LpSched::NIT, LpSched::NIT, LpSched::PF, LpSched::SYNC,
         LpSched::first_group(), LpSched::NT, LpSched::A_STEP);
  for (int np = 3; np >= 1; --np) dump_lp(np);
  printf("lg_lds STAGE=%d LO=%d TP_LD=%d TP_BYTES=%d PAR_OFF=%d BIAS_OFF=%d TP_OFF=%d PBIAS_OFF=%d LDS=%d\n", LG_STAGE, LG_LO, LG_TP_LD, LG_TP_BYTES,
         LG_PAR_OFF, LG_BIAS_OFF, LG_TP_OFF, LG_PBIAS_OFF, LG_LDS);

  printf("ao_lds KH=%d VH=%d RING=%d SLOT=%d LO=%d LDS=%d UNIT=%d\n", AO_KH, AO_VH, AO_RING, AO_SLOT, AO_LO, AO_LDS, AO_UNIT);
  bool seen_k[64] = {}, seen_v[64] = {};
  for (unsigned l = 0; l < 64; ++l) {
    printf("ao_lane lane=%u voff_k=%u voff_v=%u a_k0=%u a_k1=%u a_row=%u\n", l, ao_voff_k(l), ao_voff_v(l), ao_a_k(l, 0), ao_a_k(l, 1), ao_a_row(l));
    // a DMA piece is 1 KiB = 64 chunks of 16 bytes: the source offsets of its 64 lanes are a permutation of them
    CHECK(ao_voff_k(l) % 16 == 0 && ao_voff_k(l) < 1024 && !seen_k[ao_voff_k(l) / 16], "voff_k(%u)", l);
    CHECK(ao_voff_v(l) % 16 == 0 && ao_voff_v(l) < 1024 && !seen_v[ao_voff_v(l) / 16], "voff_v(%u)", l);
    seen_k[ao_voff_k(l) / 16] = seen_v[ao_voff_v(l) / 16] = true;
    for (unsigned r = 0; r < 32; ++r) CHECK(ao_row_chunk(ao_row_chunk(l, r), r) == l && ao_row_chunk(l, r) < 64, "row_chunk(%u, %u)", l, r);
  }
  for (unsigned q = 0; q < 128; ++q)
    for (unsigned g = 0; g < 2; ++g) CHECK(ao_voff_q(q, g) == q * 64 + g * 16, "voff_q(%u, %u)", q, g);
  // the ring as the head loop walks it: `slot` is the only state, every stage and refill is named relative to it
  int slot = 0;
  for (int h = 0; h < 8; ++h) {
    printf("ao_ring h=%d slot=%d st0=%d st1=%d st2=%d st3=%d", h, slot, ao_slot_at(slot, 0), ao_slot_at(slot, 1), ao_slot_at(slot, 2), ao_slot_at(slot, 3));
    printf(" refill_bd1=%d refill_bd2=%d refill_bd3=%d", ao_slot_at(slot, 3), ao_slot_at(slot, 4), ao_slot_at(slot, 5));   // W_h,3  W_h+1,0  W_h+1,1
    slot = ao_slot_next(slot);
    printf(" refill_ba=%d\n", ao_slot_at(slot, 2));                                                                          // W_h+1,2
  }
  printf("ao_wait Ba=%d Bb=%d Bc=%d Bd1=%d Bd2=%d Bd3=%d\n", AO_WAIT_BA, AO_WAIT_BB, AO_WAIT_BC, AO_WAIT_BD1, AO_WAIT_BD2, AO_WAIT_BD3);
  printf("OK: schedule tables of ldm_x3_sched.h dumped\n");
  return 0;
}
