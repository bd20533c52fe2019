// files_lookup_lds.hpp -- the other form of csrc/files_walk.hip's row lookup, included there in place of the
// shipped one by an ablation build (tools/build_alt.sh files_lds -DPPFS_FILES_LOOKUP_LDS=1):
// the workgroup finds the rows of its first and last entry once, loads those at most 256 rows into LDS (rows
// start at distinct entries, so 256 entries span at most 256 rows), and the lanes search there.
// Measured beside the shipped form (every lane searching global memory) on both workloads of DESIGN.md section
// 4.11: 0.6 to 2.2 % slower, within the runs' spread -- two lanes still walk the global table, and the barriers
// and the LDS search come on top.
//
// Included inside namespace ppfs, after FilesTables and Owner.
constexpr bool kOwnerAllLanes = true; // barriers: every lane of the workgroup must call
__device__ inline Owner owner_of(const FilesTables& tb, uint64_t w0, uint64_t wn, uint64_t e, bool want)
{
    __shared__ Row win[256];
    __shared__ uint64_t edge[2];
    Row r { 0, 0xFFFFFFFFu, 0 };
    __syncthreads(); // the previous pass is done with win and edge
    if (threadIdx.x == 0)
        edge[0] = filesplan::row_of(tb.rows, tb.nrows, w0);
    if (threadIdx.x == 64)
        edge[1] = filesplan::row_of(tb.rows, tb.nrows, w0 + wn - 1u);
    __syncthreads();
    const uint64_t r0 = edge[0], cnt = edge[1] - r0 + 1u;
    const bool fits = cnt <= 256u && r0 + cnt <= tb.nrows;
    if (fits && threadIdx.x < cnt && PPFS_DBG_OK(tb.rows + r0 + threadIdx.x, 16, tb.rows, tb.nrows * 16))
        win[threadIdx.x] = tb.rows[r0 + threadIdx.x];
    __syncthreads();
    if (want && fits)
        r = win[filesplan::row_of(win, cnt, e)];
    Owner o;
    o.file = r.file;
    o.ok = want && r.file < tb.nfiles && r.first <= e && PPFS_DBG_OK(tb.recs + r.file, 128, tb.recs, tb.nfiles * 128);
    o.k = e - r.first;
    return o;
}
