// OptTables (sgv_ew.h): the one host-side builder of the descriptor and work-item tables that drive the multi-tensor spectral-norm and
// AdamW kernels of optim.hip.  Everything above upload_bytes is plain host code (tests/opt_tables_host.hip runs it without a device).
#include "sgv_ew.h"
#include <algorithm>

static void emit(std::vector<WorkItem>& list, int desc, long n) { for (long c = 0; c < n; ++c) list.push_back({desc, (int)c}); }

int OptTables::add_sn(const SNDesc& d, bool skip_in_reuse, bool flat_dot, int group) {
    const int si = (int)sn.size();
    sn.push_back(d);
    if (d.active) {
        emit(items[SN], si, sn_gemv_items(d.taps, d.rows, d.cols));
        if (!skip_in_reuse) emit(items[SN_UNF], si, sn_gemv_items(d.taps, d.rows, d.cols));
        emit(items[TSUM], si, sn_tsum_items(d.taps, d.cols));
        emit(items[SSUM], si, sn_ssum_items(d.rows));
    }
    if (flat_dot) {
        const long nch = opt_flat_items((long)d.taps * d.rows * d.cols);
        fin.push_back({nullptr, d.dot, (int)nch, 0});
        fin_group.push_back(group);
        emit(items[DOT], si, nch);
        dot_group.resize(items[DOT].size(), group);
    }
    return si;
}

int OptTables::add_adam(const AdamDesc& a, bool tiled, int group) {
    const int id = (int)adam.size();
    adam.push_back(a);
    if (!a.g) return id;
    emit(items[ADAM], id, opt_flat_items(a.n));
    std::vector<WorkItem>& pass = items[tiled ? TILE : FLAT];
    emit(pass, id, tiled ? opt_tile_items(a.taps, a.rows, a.cols) : opt_flat_items(a.n));
    (tiled ? tile_group : flat_group).resize(pass.size(), group);
    return id;
}

void OptTables::add_copy(int adam_id) {
    const AdamDesc& a = adam[adam_id];
    emit(items[COPY], adam_id, opt_copy_items(a.taps, a.rows, a.cols));
}

// stable counting sort of `list` by group; off[g] = first element of group g, off[n_groups] = size
template <typename T> static void sort_by_group(std::vector<T>& list, std::vector<int>& group, int n_groups, std::vector<int>& off) {
    off.assign(n_groups + 1, 0);
    for (int g : group) off[g + 1] += 1;
    for (int g = 0; g < n_groups; ++g) off[g + 1] += off[g];
    std::vector<int> next(off.begin(), off.end() - 1);
    std::vector<T> sorted(list.size());
    for (size_t i = 0; i < list.size(); ++i) sorted[next[group[i]]++] = list[i];
    list.swap(sorted);
    group.clear();
}

void OptTables::finish(int n_groups) {
    sort_by_group(items[DOT], dot_group, n_groups, dot_off);
    sort_by_group(fin, fin_group, n_groups, fin_off);
    sort_by_group(items[FLAT], flat_group, n_groups, flat_off);
    sort_by_group(items[TILE], tile_group, n_groups, tile_off);
    // both sorts are stable, so the FinDot entries still tile the DOT list in order: src is the running sum of the counts
    size_t first = 0;
    for (auto& f : fin) { f.src = (const float*)(uintptr_t)first; first += f.count; }
}

// ---- device side ----------------------------------------------------------------------------------------------------------------
bool upload_bytes(const void* src, size_t bytes, void** dst) {
    *dst = nullptr;
    if (bytes == 0) return true;
    return hipMalloc(dst, bytes) == hipSuccess && hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
}

bool OptTables::upload(int part_fill_byte) {
    if (!upload_vec(sn, &sn_dev) || !upload_vec(adam, &adam_dev)) return false;
    for (int l = 0; l < N_LISTS; ++l) if (!upload_vec(items[l], &dev[l])) return false;
    const size_t dot_bytes = sizeof(float) * std::max<size_t>(items[DOT].size(), 1);
    const size_t gnorm_bytes = sizeof(double) * std::max<size_t>(std::max(items[FLAT].size() + items[TILE].size(), items[ADAM].size()), 1);
    if (hipMalloc((void**)&dot_part, dot_bytes) != hipSuccess || hipMemset(dot_part, part_fill_byte, dot_bytes) != hipSuccess) return false;
    if (hipMalloc((void**)&gnorm_part, gnorm_bytes) != hipSuccess || hipMemset(gnorm_part, part_fill_byte, gnorm_bytes) != hipSuccess) return false;
    for (auto& f : fin) f.src = dot_part + (uintptr_t)f.src;
    return true;
}

void OptTables::release() {
    void* ptrs[] = {sn_dev, adam_dev, dot_part, gnorm_part};
    for (void* p : ptrs) if (p) hipFree(p);
    for (WorkItem* p : dev) if (p) hipFree(p);
    *this = OptTables();
}
