// CPU access to the launch plan of a PE count (vstrains_amd/csrc/vs_pe_plan.h, product source, compiled unchanged): arrays of
// inputs in, plans out.  No device, no HIP call.  tests/test_pe_plan_cpu.py names the columns in the same order.
#include "../vstrains_amd/csrc/vs_pe_plan.h"

enum { N_IN = 30, N_OUT = 40, MSG = 128 };

// Table slots and list trim of the k_pe_tiles instantiation <mode, sw, sp, ad> (vs_std_table); `pool` = the plan's run-time pool,
// which the instantiations without a compile-time shape (sw = 0) take.  out[0] = slots, out[1] = trim.
extern "C" void vs_std_table_check(int mode, uint32_t sw, int ad, uint32_t pool, uint32_t *out) {
    const StdTable t = sw ? vs_std_table(mode, true, ad != 0) : StdTable{pool, 0u};
    out[0] = t.pool;
    out[1] = t.trim;
}

// in: n rows of N_IN values, out: n rows of N_OUT, msgs: n texts of MSG bytes.  Returns N_OUT.
extern "C" int vs_pe_plan_check(uint64_t n, const int64_t *in, uint64_t *out, char *msgs) {
    for (uint64_t i = 0; i < n; i++, in += N_IN, out += N_OUT, msgs += MSG) {
        PePlanIn a;
        a.n_nodes = (uint32_t)in[0]; a.K = (uint32_t)in[1]; a.w = (uint32_t)in[2]; a.s = (uint32_t)in[3];
        a.n_seed_pos = (uint64_t)in[4]; a.n_distinct = (uint64_t)in[5]; a.max_node_len = (uint32_t)in[6]; a.n_cu = (uint32_t)in[7];
        a.n_ends = (uint64_t)in[8]; a.max_len = (uint32_t)in[9]; a.has_mask = in[10]; a.has_inv4 = in[11];
        a.count = in[12]; a.tile_map = in[13];
        VsTuning &t = a.tune;
        t.ept = (uint32_t)in[14]; t.grid_per_cu = (uint32_t)in[15]; t.acc_fill_pct = (int)in[16]; t.shortcut = (int)in[17];
        t.adapt_grid = (int)in[18]; t.acc_rows = (int)in[19]; t.ltab_bits = (int)in[20]; t.rows_keys = (uint32_t)in[21];
        t.rows_sub = (uint32_t)in[22]; t.rows_per_strip = (uint32_t)in[23]; t.no_sort = in[24]; t.locus_global = in[25];
        t.no_fast = in[26]; t.no_std = in[27]; t.no_agg = in[28]; t.no_mid = in[29];
        const PePlan p = vs_pe_plan(a);
        const uint64_t row[N_OUT] = {(uint64_t)(int64_t)p.status, p.ept, p.pmax, p.wpe, p.pool, p.pool_bits, p.words_cap, p.magic_pmax,
                                     p.magic_wpe, p.lds_bytes, p.mode, p.sw, p.sp, p.ad, p.n_tiles, p.grid, p.list_ends, p.list_words,
                                     p.tiles_per_wg, p.shortcut, p.mid_fast, p.use_sort, p.lds_sort, p.locus_chunk, p.locus_per_pass,
                                     p.locus_keys, p.locus_hist_words, p.use_rows, p.use_table, p.mark_tiles, p.acc_grid, p.acc_per_wg,
                                     p.acc_fill, p.rows_sub_pairs, p.rows_ltab_bits, p.rows_keys, p.rows_fill, p.rows_per_strip,
                                     p.slow_grid, p.dense_bytes};
        for (int j = 0; j < N_OUT; j++) out[j] = row[j];
        for (int j = 0; j < MSG; j++) msgs[j] = p.msg[j];
    }
    return N_OUT;
}
