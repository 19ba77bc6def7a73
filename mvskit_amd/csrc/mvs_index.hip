// mvs_index.hip -- the cell index (m_pgrids / m_vpgrids as id lists behind 64-bit offsets: count, fill, sort and trim, finalize, pack),
// and the per-cell maps derived from the pool (m_dpgrids, the best-NCC map, their extraction); kernels first, their launchers behind them.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mvs_camera.cuh"
#include "mvs_common.cuh"
#include "mvs_kernels.h"

using namespace mvsdev;

// list entry of the index build: ascending key order = descending m_ncc, then ascending id (PatchManager::sortPatches)
__device__ __forceinline__ unsigned long long list_key(float ncc, int64_t id) {
    return ((unsigned long long)(~sortable_f32(ncc + 0.0f)) << 32) | (unsigned long long)(uint32_t)id;  // + 0.0f: -0 sorts as +0
}
// =================================================================== index build
// cnt[gcell] += 1 for every (patch, view) membership: PatchManager::addPatch, patch_manager.cpp:158-186
__global__ void k_index_count(DParams prm, int32_t* __restrict__ cnt, int32_t* __restrict__ vcnt, unsigned long long* __restrict__ total) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int mine = 0;  // list entries this patch adds (their sum sizes the id / key buffers)
    if (id < prm.pool_n && (prm.pool[id].flags & 1)) {
        const DPatch* p = prm.pool + id;
        const F4 coord = ld4(p->coord);
        const int n = cnt ? min(p->nimages, MVS_LISTCAP) : 0;
        for (int i = 0; i < n; ++i) {
            const DView* vw = prm.views + p->images[i];
            int ix, iy;
            cell_of(prm, vw, coord, ix, iy);
            if (ix < 0 || vw->gw <= ix || iy < 0 || vw->gh <= iy) continue;
            atomicAdd(&cnt[vw->cell_base + iy * vw->gw + ix], 1);
            ++mine;
        }
        if (vcnt) {
            const int nv = min(p->nvimages, MVS_LISTCAP);
            for (int i = 0; i < nv; ++i) {
                const DView* vw = prm.views + p->vimages[i];
                int ix, iy;
                cell_of(prm, vw, coord, ix, iy);
                if (ix < 0 || vw->gw <= ix || iy < 0 || vw->gh <= iy) continue;
                atomicAdd(&vcnt[vw->cell_base + iy * vw->gw + ix], 1);
                ++mine;
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
    if (total && (threadIdx.x & 63) == 0 && mine) atomicAdd(total, (unsigned long long)mine);  // (the index build reads the sum off its scan instead)
}
// one grid per launch (vgrid = 0: m_pgrids from m_images, 1: m_vpgrids from m_vimages): the sort key travels with the id, the per-cell
// sort reads no patch
__global__ void k_index_fill(DParams prm, int vgrid, const csr_off_t* __restrict__ start, int32_t* __restrict__ cursor, unsigned long long* __restrict__ ids) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= prm.pool_n) return;
    const DPatch* p = prm.pool + id;
    if (!(p->flags & 1)) return;
    const F4 coord = ld4(p->coord);
    const unsigned long long key = list_key(p->ncc, id);
    const int n = vgrid ? min(p->nvimages, MVS_LISTCAP) : min(p->nimages, MVS_LISTCAP);
    for (int i = 0; i < n; ++i) {
        const DView* vw = prm.views + (vgrid ? p->vimages[i] : p->images[i]);
        int ix, iy;
        cell_of(prm, vw, coord, ix, iy);
        if (ix < 0 || vw->gw <= ix || iy < 0 || vw->gh <= iy) continue;
        const int g = vw->cell_base + iy * vw->gw + ix;
        ids[start[g] + atomicAdd(&cursor[g], 1)] = key;
    }
}
// The index between the stages of Filter::run: no trim, and no stage depends on the order inside a list (computeGain takes maxima,
// findNeighbors builds a set whose layout is the same for every insertion order, filterSmallGroups joins sets), so the thread that
// holds the record writes the finished entry straight into its slot: no keys, no per-cell sort, no gather of the records.
// (The entry is the id; no reader inside Filter::run looks at csr_key.)
__global__ void k_index_fill_direct(DParams prm, int vgrid, const csr_off_t* __restrict__ start, int32_t* __restrict__ cursor, int32_t* __restrict__ id32) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= prm.pool_n) return;
    const DPatch* p = prm.pool + id;
    if (!(p->flags & 1)) return;
    const F4 coord = ld4(p->coord);
    const int n = vgrid ? min(p->nvimages, MVS_LISTCAP) : min(p->nimages, MVS_LISTCAP);
    for (int i = 0; i < n; ++i) {
        const DView* vw = prm.views + (vgrid ? p->vimages[i] : p->images[i]);
        int ix, iy;
        cell_of(prm, vw, coord, ix, iy);
        if (ix < 0 || vw->gw <= ix || iy < 0 || vw->gh <= iy) continue;
        const int g = vw->cell_base + iy * vw->gw + ix;
        const csr_off_t slot = start[g] + atomicAdd(&cursor[g], 1);
        id32[slot] = (int32_t)id;
    }
}
// PatchManager::sortPatches (descending NCC; ties by id) per cell, then the MAX_NUM_OF_PATCHES trim
// (propagate.cpp:94-99,130-135): every cell decides on the same snapshot; a trimmed patch dies everywhere.
__global__ void k_index_sort_trim(DParams prm, const csr_off_t* __restrict__ start, unsigned long long* __restrict__ ids, int do_trim,
                                  unsigned long long* __restrict__ trimmed) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = g < prm.total_cells;
    const csr_off_t b = in ? start[g] : 0, e = in ? start[g + 1] : 0;
    for (csr_off_t i = b + 1; i < e; ++i) {  // insertion sort, ascending keys
        const unsigned long long k = ids[i];
        csr_off_t j = i - 1;
        while (j >= b) {
            const unsigned long long o = ids[j];
            if (o < k) break;
            ids[j + 1] = o;
            --j;
        }
        ids[j + 1] = k;
    }
    if (do_trim) {
        int mine = 0;
        for (csr_off_t k = b + prm.cap; k < e; ++k) {
            const int old = atomicAnd(&prm.pool[(uint32_t)ids[k]].flags, ~1);
            mine += old & 1;
        }
        // one counter update per wave, not per trimmed patch, and into one of 256 partial sums (waves that end on an atomic to ONE
        // address leave in single file: the host adds the partial sums)
        for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(trimmed + (blockIdx.x & 255u), (unsigned long long)mine);
    }
}
// After the trim: every list is compacted to its alive entries (order kept) at the FRONT of its own range -- the id to id32, the
// (m_ncc, reference view) key of an m_pgrids entry over the sort key it replaces (a cell's thread reads position k >= b + n before it
// writes position b + n) -- and counted.  k_index_pack then closes the gaps the trim left between the lists.
__global__ void k_index_finalize(DParams prm, int vgrid, const csr_off_t* __restrict__ start, unsigned long long* __restrict__ ids,
                                 int32_t* __restrict__ id32, int32_t* __restrict__ cnt_alive) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= prm.total_cells) return;
    const csr_off_t b = start[g], e = start[g + 1];
    int n = 0;
    for (csr_off_t k = b; k < e; ++k) {
        const int id = (int)(uint32_t)ids[k];
        const DPatch* p = prm.pool + id;
        if (!(p->flags & 1)) continue;
        if (!vgrid) ids[b + n] = ((unsigned long long)(uint32_t)p->images[0] << 32) | (unsigned long long)__float_as_uint(p->ncc);  // m_vpgrids' readers want ids only
        id32[b + n] = id;
        ++n;
    }
    cnt_alive[g] = n;
}
// The lists of neighbouring cells end to end (start2 = the scan of the alive counts): Optim::check's findNeighbors reads the cells of a
// grid row as ONE run of ids, which the gaps the trim left would break.
__global__ void k_index_pack(DParams prm, const csr_off_t* __restrict__ start, const csr_off_t* __restrict__ start2, const int32_t* __restrict__ cnt_alive,
                             const unsigned long long* __restrict__ ids, const int32_t* __restrict__ id32_in, ListKey* __restrict__ key, int32_t* __restrict__ id32_out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= prm.total_cells) return;
    const csr_off_t b = start[g], b2 = start2[g];
    const int n = cnt_alive[g];
    for (int k = 0; k < n; ++k) {
        id32_out[b2 + k] = id32_in[b + k];
        if (key) {
            const unsigned long long w = ids[b + k];
            ListKey lk;
            lk.ncc = __uint_as_float((uint32_t)w); lk.ref = (int32_t)(w >> 32);
            key[b2 + k] = lk;
        }
    }
}
// PatchManager::updateDepthMaps, patch_manager.cpp:191-221, over the alive pool (Filter::setDepthMaps, filter.cpp:580-626)
// A lane per patch, a wave per view (the four waves of a block share 64 consecutive patches and take the views in turn): patches that
// follow each other in the pool lie next to each other on the surface, so the 64 cells a wave touches in one view's map share
// cache lines -- with a lane per (patch, view) pair every lane of a wave wrote into another view's map.
// `dirty` (one bit per cell, or null): only the cells whose nearest patch a filter stage has just removed are recomputed
// (k_depth_mark_dirty emptied them); every other cell's nearest patch is still alive, so its entry stands.
__global__ __launch_bounds__(256) void k_depth_maps(DParams prm, unsigned long long* __restrict__ dp, const uint32_t* __restrict__ dirty) {
    const int64_t id = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63u);
    if (id >= prm.pool_n) return;
    const DPatch* p = prm.pool + id;
    if (!(p->flags & 1)) return;
    const F4 coord = ld4(p->coord);
    for (int image = (int)(threadIdx.x >> 6); image < prm.nviews; image += 4) {
        const DView* vw = prm.views + image;
        const F3 ic = project(vw, coord, prm.level);
        const float fx = ic.x / (float)prm.csize, fy = ic.y / (float)prm.csize;
        const int xs[2] = {(int)floorf(fx), (int)ceilf(fx)}, ys[2] = {(int)floorf(fy), (int)ceilf(fy)};
        const float depth = dot4(ld4(vw->oaxis), coord);
        const unsigned long long key = ((unsigned long long)sortable_f32(depth) << 32) | (unsigned long long)(uint32_t)id;
        for (int j = 0; j < 2; ++j) for (int i = 0; i < 2; ++i) {
            if (xs[i] < 0 || vw->gw <= xs[i] || ys[j] < 0 || vw->gh <= ys[j]) continue;
            if (i == 1 && xs[1] == xs[0]) continue;  // same cell twice: idempotent, skip
            if (j == 1 && ys[1] == ys[0]) continue;
            // the cell's value only ever decreases: a plain read that already shows a nearer patch saves the atomic (most do)
            const int cell = vw->cell_base + ys[j] * vw->gw + xs[i];
            if (dirty && !((dirty[cell >> 5] >> (cell & 31)) & 1u)) continue;
            unsigned long long* cellp = &dp[cell];
            if (key < __builtin_nontemporal_load(cellp)) atomicMin(cellp, key);
        }
    }
}
// Before a filter stage's removals are applied: the cells of the depth maps that name a patch about to go are emptied and marked.
// (A cell names one patch, so only that patch's thread writes it.)
__global__ __launch_bounds__(256) void k_depth_mark_dirty(DParams prm, const uint8_t* __restrict__ kill, unsigned long long* __restrict__ dp, uint32_t* __restrict__ dirty) {
    const int64_t id = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63u);
    if (id >= prm.pool_n || !kill[id]) return;
    const DPatch* p = prm.pool + id;
    if (!(p->flags & 1)) return;
    const F4 coord = ld4(p->coord);
    for (int image = (int)(threadIdx.x >> 6); image < prm.nviews; image += 4) {
        const DView* vw = prm.views + image;
        const F3 ic = project(vw, coord, prm.level);
        const float fx = ic.x / (float)prm.csize, fy = ic.y / (float)prm.csize;
        const int xs[2] = {(int)floorf(fx), (int)ceilf(fx)}, ys[2] = {(int)floorf(fy), (int)ceilf(fy)};
        for (int j = 0; j < 2; ++j) for (int i = 0; i < 2; ++i) {
            if (xs[i] < 0 || vw->gw <= xs[i] || ys[j] < 0 || vw->gh <= ys[j]) continue;
            if (i == 1 && xs[1] == xs[0]) continue;
            if (j == 1 && ys[1] == ys[0]) continue;
            const int cell = vw->cell_base + ys[j] * vw->gw + xs[i];
            if ((uint32_t)(dp[cell] & 0xffffffffull) != (uint32_t)id) continue;
            dp[cell] = ~0ull;
            atomicOr(&dirty[cell >> 5], 1u << (cell & 31));
        }
    }
}
// best-NCC patch per cell among those whose reference view is `view` (parity artefact)
__global__ void k_best_ncc_map(DParams prm, int view, unsigned long long* __restrict__ best) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= prm.pool_n) return;
    const DPatch* p = prm.pool + id;
    if (!(p->flags & 1) || p->nimages == 0 || p->images[0] != view) return;
    const DView* vw = prm.views + view;
    int ix, iy;
    cell_of(prm, vw, ld4(p->coord), ix, iy);
    if (ix < 0 || vw->gw <= ix || iy < 0 || vw->gh <= iy) return;
    const unsigned long long key = ((unsigned long long)sortable_f32(p->ncc) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)id);
    atomicMax(&best[iy * vw->gw + ix], key);
}
__global__ void k_map_extract(DParams prm, int view, int kind, const unsigned long long* __restrict__ sel, float* __restrict__ depth,
                              float* __restrict__ normal, int32_t* __restrict__ ids, int ncells) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    const unsigned long long k = sel[c];
    const bool empty = kind == 0 ? (k == ~0ull) : (k == 0ull);
    if (empty) {
        depth[c] = __int_as_float(0x7fc00000);
        normal[3 * c] = normal[3 * c + 1] = normal[3 * c + 2] = __int_as_float(0x7fc00000);
        ids[c] = -1;
        return;
    }
    const uint32_t id = kind == 0 ? (uint32_t)(k & 0xffffffffull) : 0xffffffffu - (uint32_t)(k & 0xffffffffull);
    const DPatch* p = prm.pool + id;
    depth[c] = dot4(ld4((prm.views + view)->oaxis), ld4(p->coord));
    normal[3 * c] = p->normal[0]; normal[3 * c + 1] = p->normal[1]; normal[3 * c + 2] = p->normal[2];
    ids[c] = (int32_t)id;
}

// =================================================================== host-callable launchers
void mvsk_index_count(const DParams& prm, int32_t* cnt, int32_t* vcnt, unsigned long long* total, hipStream_t st) {
    if (prm.pool_n > 0) hipLaunchKernelGGL(k_index_count, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, prm, cnt, vcnt, total);
}
void mvsk_index_fill(const DParams& prm, int vgrid, const csr_off_t* start, int32_t* cursor, unsigned long long* ids, hipStream_t st) {
    if (prm.pool_n > 0) hipLaunchKernelGGL(k_index_fill, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, prm, vgrid, start, cursor, ids);
}
void mvsk_index_fill_direct(const DParams& prm, int vgrid, const csr_off_t* start, int32_t* cursor, int32_t* id32, hipStream_t st) {
    if (prm.pool_n > 0) hipLaunchKernelGGL(k_index_fill_direct, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, prm, vgrid, start, cursor, id32);
}
void mvsk_index_sort_trim(const DParams& prm, const csr_off_t* start, unsigned long long* ids, int do_trim, unsigned long long* trimmed, hipStream_t st) {
    hipLaunchKernelGGL(k_index_sort_trim, dim3(nblk(prm.total_cells, 256)), dim3(256), 0, st, prm, start, ids, do_trim, trimmed);
}
void mvsk_index_finalize(const DParams& prm, int vgrid, const csr_off_t* start, unsigned long long* ids, int32_t* id32, int32_t* cnt_alive, hipStream_t st) {
    hipLaunchKernelGGL(k_index_finalize, dim3(nblk(prm.total_cells, 256)), dim3(256), 0, st, prm, vgrid, start, ids, id32, cnt_alive);
}
void mvsk_index_pack(const DParams& prm, const csr_off_t* start, const csr_off_t* start2, const int32_t* cnt_alive, const unsigned long long* ids, const int32_t* id32_in,
                     ListKey* key, int32_t* id32_out, hipStream_t st) {
    hipLaunchKernelGGL(k_index_pack, dim3(nblk(prm.total_cells, 256)), dim3(256), 0, st, prm, start, start2, cnt_alive, ids, id32_in, key, id32_out);
}
void mvsk_depth_maps(const DParams& prm, unsigned long long* dp, const uint32_t* dirty, hipStream_t st) {
    if (prm.pool_n > 0) hipLaunchKernelGGL(k_depth_maps, dim3(nblk(prm.pool_n, 64)), dim3(256), 0, st, prm, dp, dirty);
}
void mvsk_depth_mark_dirty(const DParams& prm, const uint8_t* kill, unsigned long long* dp, uint32_t* dirty, hipStream_t st) {
    if (prm.pool_n > 0) hipLaunchKernelGGL(k_depth_mark_dirty, dim3(nblk(prm.pool_n, 64)), dim3(256), 0, st, prm, kill, dp, dirty);
}
void mvsk_best_ncc_map(const DParams& prm, int view, unsigned long long* best, hipStream_t st) {
    if (prm.pool_n > 0) hipLaunchKernelGGL(k_best_ncc_map, dim3(nblk(prm.pool_n, 256)), dim3(256), 0, st, prm, view, best);
}
void mvsk_map_extract(const DParams& prm, int view, int kind, const unsigned long long* sel, float* depth, float* normal, int32_t* ids, int ncells, hipStream_t st) {
    hipLaunchKernelGGL(k_map_extract, dim3(nblk(ncells, 256)), dim3(256), 0, st, prm, view, kind, sel, depth, normal, ids, ncells);
}
