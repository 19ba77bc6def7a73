// mvs_mesh_attr_colours.cuh -- the body of the two colour kernels of mvs_mesh_attr.hip, which includes it twice: between the braces of
// k_mattr_colours with MATTR_GATED 0 and of k_mattr_colours_visible with MATTR_GATED 1 (view v takes part for vertex i only when bit v
// of visible[i] is set).  As text and not as a function: an inlined function's __restrict__ arguments are not a kernel's, and
// k_mattr_colours would not keep the machine code it had ("f-12 mesh render").  No include guard, nothing but the body.
// prm, a, m, n_v, verts, normals, ids, usable, rgb, used (and visible) are the kernel's arguments.
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool live = i < n_v;  // a lane beyond the end stays for the shuffles of the packed store
    uint32_t colour = 128u | 128u << 8 | 128u << 16, use = 0u;
    if (live) {
        const F3 X = ld3(verts + 3 * i);
        const F4 X1{X.x, X.y, X.z, 1.0f};
        const F3 n = normals ? ld3(normals + 3 * i) : F3{0.0f, 0.0f, 0.0f};
        const bool facing = !(n.x == 0.0f && n.y == 0.0f && n.z == 0.0f);  // a NaN normal is tested, and fails
        // tier 0: the CONFIRMED views, tier 1: the UNCONFIRMED ones
        float sw[2] = {0.0f, 0.0f}, sr[2] = {0.0f, 0.0f}, sg[2] = {0.0f, 0.0f}, sb[2] = {0.0f, 0.0f};
        int cnt[2] = {0, 0};
#if MATTR_GATED
        const u64 vis = visible[i];
#endif
        for (int v = 0; v < prm.nviews; ++v) {
#if MATTR_GATED
            if (!((vis >> v) & 1ull)) continue;
#endif
            const DView* vw = prm.views + v;
            const int W = vw->W[prm.level], H = vw->H[prm.level];
            const F3 ic = project(vw, X1, prm.level);
            if (!(ic.z > 0.0f && ic.x >= 0.0f && ic.y >= 0.0f && ic.x < (float)(W - 1) && ic.y < (float)(H - 1))) continue;
            const int64_t near = (int64_t)(int)floorf(ic.y + 0.5f) * W + (int)floorf(ic.x + 0.5f);  // inside the image: the window is
            if (vw->mask && vw->mask[near] == 0) continue;
            const F4 C = ld4(vw->center);
            float w = 1.0f;
            if (facing) {
                const F3 d{C.x - X.x, C.y - X.y, C.z - X.z};
                w = dot3(n, d) / sqrtf(dot3(d, d));
                if (!(w >= m.min_cos)) continue;
            }
            int tier = 1;
            const int64_t pix = a.pix_base[v] + near;
            const int32_t idq = usable[pix] ? ids[pix] : -1;
            if (idq >= 0 && (int64_t)idq < prm.pool_n) {
                const DPatch* q = prm.pool + idq;
                const F4 X0q = ld4(q->coord), nq4 = ld4(q->normal);
                const F3 nq{nq4.x, nq4.y, nq4.z};
                const float den = dot3(nq, F3{X.x - C.x, X.y - C.y, X.z - C.z});
                const float num = dot3(nq, F3{X0q.x - C.x, X0q.y - C.y, X0q.z - C.z});
                if (!mattr_finite_nonzero(den)) continue;
                const float s = num / den;
                if (!(fabsf(s - 1.0f) <= m.occl_tol)) continue;  // occluded behind that view's surface, or floating in front of it
                tier = 0;
            }
            // ply_colour's bilinear sample of the RGBA8 pyramid, its expressions in its order
            const float x = ic.x, y = ic.y;
            const int lx = (int)x, ly = (int)y;
            const float dx1 = x - lx, dx0 = 1.0f - dx1, dy1 = y - ly, dy0 = 1.0f - dy1;
            const float f00 = dx0 * dy0, f01 = dx0 * dy1, f10 = dx1 * dy0, f11 = dx1 * dy1;
            const uint32_t* r0 = vw->img[prm.level] + ((size_t)ly * W + lx);
            const uint32_t* r1 = r0 + W;
            const uint32_t ta = r0[0], tb = r0[1], tc = r1[0], td = r1[1];
#define MATTR_CH(t, s) ((int)(((t) >> (s)) & 0xffu))
            const float cr = (MATTR_CH(ta, 0) * f00 + MATTR_CH(tc, 0) * f01) + (MATTR_CH(tb, 0) * f10 + MATTR_CH(td, 0) * f11);
            const float cg = (MATTR_CH(ta, 8) * f00 + MATTR_CH(tc, 8) * f01) + (MATTR_CH(tb, 8) * f10 + MATTR_CH(td, 8) * f11);
            const float cb = (MATTR_CH(ta, 16) * f00 + MATTR_CH(tc, 16) * f01) + (MATTR_CH(tb, 16) * f10 + MATTR_CH(td, 16) * f11);
#undef MATTR_CH
            // the tier is a select, not an index: the sums stay in registers
            const bool t0 = tier == 0;
            sw[0] = t0 ? sw[0] + w : sw[0]; sr[0] = t0 ? sr[0] + w * cr : sr[0]; sg[0] = t0 ? sg[0] + w * cg : sg[0]; sb[0] = t0 ? sb[0] + w * cb : sb[0];
            sw[1] = t0 ? sw[1] : sw[1] + w; sr[1] = t0 ? sr[1] : sr[1] + w * cr; sg[1] = t0 ? sg[1] : sg[1] + w * cg; sb[1] = t0 ? sb[1] : sb[1] + w * cb;
            cnt[0] += t0 ? 1 : 0; cnt[1] += t0 ? 0 : 1;
        }
        if (cnt[0] > 0) {
            colour = mattr_channel(sr[0], sw[0]) | mattr_channel(sg[0], sw[0]) << 8 | mattr_channel(sb[0], sw[0]) << 16;
            use = (uint32_t)cnt[0] | 0x80u;
        } else if (cnt[1] > 0) {
            colour = mattr_channel(sr[1], sw[1]) | mattr_channel(sg[1], sw[1]) << 8 | mattr_channel(sb[1], sw[1]) << 16;
            use = (uint32_t)cnt[1];
        }
    }
    if (live && used) used[i] = (uint8_t)use;
    // the twelve bytes of lanes 4 g .. 4 g + 3 as three words, written by the first three of them: the block starts at a multiple of four
    // vertices, so a 4-byte aligned rgb has every quad on a word boundary
    const int lane = lane_id(), quad = lane & ~3, j = lane & 3;
    const uint32_t c0 = (uint32_t)__shfl((int)colour, quad), c1 = (uint32_t)__shfl((int)colour, quad + 1), c2 = (uint32_t)__shfl((int)colour, quad + 2),
                   c3 = (uint32_t)__shfl((int)colour, quad + 3);
    const bool packed = (reinterpret_cast<uintptr_t>(rgb) & 3u) == 0u && (i - j) + 3 < n_v;
    if (packed) {
        const uint32_t word = j == 0 ? (c0 | c1 << 24) : (j == 1 ? (c1 >> 8 | c2 << 16) : (c2 >> 16 | c3 << 8));
        if (j < 3) reinterpret_cast<uint32_t*>(rgb + 3 * (i - j))[j] = word;
    } else if (live) {
        rgb[3 * i] = (uint8_t)(colour & 0xffu);
        rgb[3 * i + 1] = (uint8_t)((colour >> 8) & 0xffu);
        rgb[3 * i + 2] = (uint8_t)((colour >> 16) & 0xffu);
    }
