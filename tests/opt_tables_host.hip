// Stand-alone driver of the host-side table builder (OptTables, csrc/sgv_ew.h) for tests/test_opt_tables_host.py: builds the tables over a
// host buffer that stands in for device memory (nothing is uploaded, no HIP call is made) and prints them as text.
// Arguments: the number of groups, then one "taps,rows,cols,active,tiled,group,copy" per entry; rows = 0 is a plain tensor of `cols`
// elements.  A spectrally-normalised entry that is not tiled gets its <G,W> from the flat pass, as in the sgv_test_optset hook.
#include "../simulgen-vae_amd/csrc/sgv_ew.h"
#include "../simulgen-vae_amd/csrc/opt_tables.hip"

#include <stdio.h>
#include <stdlib.h>

struct Entry { int taps, rows, cols, active, tiled, group, copy; };

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int n_groups = atoi(argv[1]);
    std::vector<Entry> entries;
    size_t total = 0;
    for (int i = 2; i < argc; ++i) {
        Entry e;
        if (sscanf(argv[i], "%d,%d,%d,%d,%d,%d,%d", &e.taps, &e.rows, &e.cols, &e.active, &e.tiled, &e.group, &e.copy) != 7) return 2;
        if (e.rows > 0) total += sn_scratch_floats(e.taps, e.rows, e.cols);
        entries.push_back(e);
    }
    float* scratch = (float*)aligned_alloc(16, std::max<size_t>(total, 4) * sizeof(float));
    std::vector<float> dots(entries.size() * SGV_DOT_SLOTS), grad(4);
    float* cursor = scratch;
    OptTables t;
    for (size_t i = 0; i < entries.size(); ++i) {
        const Entry& e = entries[i];
        AdamDesc a = {};
        a.g = grad.data(); a.n = e.rows > 0 ? (long)e.taps * e.rows * e.cols : e.cols; a.sn = -1; a.taps = 1; a.rows = 1; a.cols = (int)a.n;
        if (e.rows > 0) {
            SNDesc d = {};
            d.taps = e.taps; d.rows = e.rows; d.cols = e.cols; d.active = e.active;
            d.dot = dots.data() + i * SGV_DOT_SLOTS;
            sn_scratch_carve(d, cursor);
            a.sn = t.add_sn(d, e.tiled != 0, !e.tiled, e.group);
            a.taps = e.taps; a.rows = e.rows; a.cols = e.cols;
            printf("sn %d entry %zu scratch %td %td %td %td\n", a.sn, i, d.tmp_t - scratch, d.tmp_s - scratch, d.tpart - scratch, d.spart - scratch);
        }
        const int id = t.add_adam(a, e.tiled != 0, e.group);
        if (e.copy) t.add_copy(id);
        printf("adam %d entry %zu sn %d\n", id, i, a.sn);
    }
    t.finish(n_groups);
    static const char* names[OptTables::N_LISTS] = {"sn", "sn_unf", "tsum", "ssum", "dot", "adam", "flat", "tile", "copy"};
    for (int l = 0; l < OptTables::N_LISTS; ++l)
        for (const WorkItem& w : t.items[l]) printf("item %s %d %d\n", names[l], w.desc, w.chunk);
    const std::vector<int>* offs[] = {&t.dot_off, &t.fin_off, &t.flat_off, &t.tile_off};
    static const char* off_names[] = {"dot", "fin", "flat", "tile"};
    for (int k = 0; k < 4; ++k) {
        printf("off %s", off_names[k]);
        for (int o : *offs[k]) printf(" %d", o);
        printf("\n");
    }
    for (const FinDot& f : t.fin) printf("fin entry %td src %zu count %d\n", (f.dst - dots.data()) / SGV_DOT_SLOTS, (size_t)(uintptr_t)f.src, f.count);
    printf("scratch base_mod16 %zu end %td total %zu\n", (size_t)((uintptr_t)scratch & 15), cursor - scratch, total);
    free(scratch);
    return 0;
}
