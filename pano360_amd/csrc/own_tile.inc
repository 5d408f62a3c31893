// One instance of the two-level ownership kernel for OW_SUBS sub-tiles (64 x 16) per workgroup:
// included by blend.hip once per tile height, with OW_FN(name) giving the instance's names.
// (The common definitions - OW_T, OW_Q, OW_CAMS, OW_QLIST, OW_ILP, the fill codes - stand in
// blend.hip in front of the first inclusion.)
#define OW_TH (OW_Q * OW_SUBS)      // the tile is 64 x (16 OW_SUBS) pixels
#define OW_NQ (4 * OW_SUBS)         // quarters per tile

struct OW_FN(OwnShared) {
    CamList cl;
    pano_camera cam[OW_CAMS];
    double sn[OW_T], cs[OW_T], tn[OW_TH];        // the tile's columns / rows (clamped to the strip / H)
    double rq[4][4];                            // per quarter column: s_lo, s_hi, c_lo, c_hi
    double rall[4];                             // the same over all 64 columns
    double step2;                               // squared chord of the unit circle between two adjacent columns
    double rsub[OW_SUBS][2];                        // per sub-tile (16 rows): t_lo, t_hi
    int low1[OW_SUBS], ncand[OW_SUBS];                    // level 1: largest lower bound (float bits), survivors
    int subfill[OW_SUBS];                                 // the camera that owns a whole sub-tile, or -1
    float hi2[OW_NQ][OW_QLIST];                    // level 2: upper bounds of the sub-tile's survivors
    int low2[OW_NQ];
    short qlist[OW_NQ][OW_QLIST];                  // level 2: survivors' list positions, in order
    int qn[OW_NQ];                               // their number; -1: the sub-tile's list; -2: the whole list
    int qfill[OW_NQ];                             // camera that owns the whole quarter, OW_NOBODY or OW_EVAL
    int evalq[OW_NQ], n_eval;
    alignas(16) short town[OW_TH][OW_T];         // evaluated quarters: owner, OW_NOBODY or OW_UNOWNED
    // behind it, sized by the host from NL = min(n, OWN_LIST) (OW_FN(own_shared_bytes)):
    //   int box[NL][4]      region search, by camera index
    //   float hi[OW_SUBS][NL]  level 1: upper bounds by list position
    //   short keep[OW_SUBS][NL] level 1: survivors' list positions, in order
};
static inline size_t OW_FN(own_shared_bytes)(int n) {
    const size_t nl = (size_t)(n < OWN_LIST ? n : OWN_LIST);
    return sizeof(OW_FN(OwnShared)) + nl * (16 + 4 * OW_SUBS + 2 * OW_SUBS) + 16;
}

// MODE: where a listed camera's record is read - 0 global memory, 1 LDS by list position,
// 2 LDS by camera index (two pointers a compiler cannot tell apart go through the flat path, so
// the tile's code exists once per mode)
template <int MODE>
__device__ __forceinline__ void OW_FN(own_tile)(OW_FN(OwnShared) &S, int (*__restrict__ s_box)[4],
                                         float *__restrict__ s_hi, short *__restrict__ s_keep, int NL,
                                         const pano_camera *__restrict__ cams, int n,
                                         int H, int W, int bx0, int bx1, int by0, int by1,
                                         int listed, int prune, int vt, int16_t *__restrict__ owner,
                                         uint8_t *__restrict__ valid, int32_t *__restrict__ boxes,
                                         int box_stride, uint8_t *__restrict__ marks) {
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    // position in the list -> camera record / camera index (listed < 0: the list overflowed, a
    // "position" is the camera's index and all n cameras are walked)
    auto index_at = [&](int pos) -> int { return listed < 0 ? pos : S.cl.list[pos]; };
    auto cam_at = [&](int pos) -> const pano_camera * {
        if (MODE == 1) return &S.cam[pos];
        if (MODE == 2) return &S.cam[index_at(pos)];
        return cams + index_at(pos);
    };

    if (listed == 0) {
        if (tid < OW_NQ) S.qfill[tid] = OW_NOBODY;
        __syncthreads();
    } else if (prune && listed > 0) {
        // ---- level 1: every listed camera on every 64 x 16 sub-tile --------------------------------
        for (int t = vt; t < OW_SUBS * listed; t += 256) {
            const int sub = t / listed, k = t - sub * listed;
            const int sy0 = by0 + OW_Q * sub, sy1 = min(sy0 + OW_Q, H);
            float hi = -1.0f;
            if (sy0 < H) {
                const double rng[6] = {S.rall[0], S.rall[1], S.rsub[sub][0], S.rsub[sub][1],
                                       S.rall[2], S.rall[3]};
                const pano_camera *cam = cam_at(k);
                // (the end columns' form when the tile spans a small angle: alpha_bound_ends)
                const int cb_ = bx1 - 1 - bx0;
                const double sa = S.sn[0], ca = S.cs[0], sb = S.sn[cb_], cb = S.cs[cb_];
                const bool narrow = (double)(cb_ * cb_) * S.step2 <= 0.0625;
                const AlphaBound bnd = narrow ? alpha_bound_ends(cam, sa, ca, sb, cb, S.rsub[sub][0], S.rsub[sub][1])
                                              : alpha_bound(cam, rng);
                hi = bnd.hi;
                // a lower bound beats the other cameras on EVERY pixel only if this camera is a
                // candidate on every pixel: the tile lies inside its patch rectangle (see above)
                if (bnd.lo > 0.0f && tile_inside(cam, bx0, bx1, sy0, sy1))
                    atomicMax(&S.low1[sub], __float_as_int(bnd.lo));
            }
            s_hi[sub * NL + k] = hi;
        }
        __syncthreads();
        for (int sub = wave; sub < OW_SUBS; sub += 4) {
            // survivors of a sub-tile, order preserved: the first maximum wins
            const float L = __int_as_float(S.low1[sub]);
            int nc = 0;
            for (int base = 0; base < listed; base += 64) {
                const int k = base + lane;
                const bool keep = k < listed && s_hi[sub * NL + k] >= L;
                const unsigned long long bal = __ballot(keep);
                if (keep) s_keep[sub * NL + nc + __popcll(bal & ((1ull << lane) - 1ull))] = (short)k;
                nc += __popcll(bal);
            }
            if (lane == 0) {
                S.ncand[sub] = nc;
                // one survivor with a positive lower bound on a sub-tile inside its rectangle owns
                // all of it: no second level for this sub-tile (most of a mosaic: the workgroups
                // away from every seam skip the second bound pass altogether)
                int whole = -1;
                if (nc == 1 && L > 0.0f) {
                    const int pos = s_keep[sub * NL];
                    const int sy0 = by0 + OW_Q * sub, sy1 = min(sy0 + OW_Q, H);
                    if (tile_inside(cam_at(pos), bx0, bx1, sy0, sy1)) whole = index_at(pos);
                }
                S.subfill[sub] = whole;
            }
        }
        __syncthreads();
        // ---- level 2: a sub-tile's survivors on its four 16 x 16 quarters ---------------------------
        int off[OW_SUBS + 1];
        off[0] = 0;
#pragma unroll
        for (int sub = 0; sub < OW_SUBS; ++sub) {
            const int nc = S.ncand[sub];
            const bool again = by0 + OW_Q * sub < H && nc >= 1 && nc <= OW_QLIST && S.subfill[sub] < 0;
            off[sub + 1] = off[sub] + (again ? 4 * nc : 0);
        }
        for (int t = vt; t < off[OW_SUBS]; t += 256) {
            int sub = 0;
#pragma unroll
            for (int u = 1; u < OW_SUBS; ++u) sub += t >= off[u] ? 1 : 0;
            const int nc = S.ncand[sub], r = t - off[sub], q = r / nc, j = r - q * nc;
            const int sy0 = by0 + OW_Q * sub, sy1 = min(sy0 + OW_Q, H);
            const int qx0 = bx0 + OW_Q * q, qx1 = min(qx0 + OW_Q, bx1);
            float hi = -1.0f;
            if (qx0 < bx1) {
                const double rng[6] = {S.rq[q][0], S.rq[q][1], S.rsub[sub][0], S.rsub[sub][1],
                                       S.rq[q][2], S.rq[q][3]};
                const pano_camera *cam = cam_at(s_keep[sub * NL + j]);
                const int ca_ = qx0 - bx0, cb_ = qx1 - 1 - bx0;
                const double sa = S.sn[ca_], ca = S.cs[ca_], sb = S.sn[cb_], cb = S.cs[cb_];
                const bool narrow = (double)((cb_ - ca_) * (cb_ - ca_)) * S.step2 <= 0.0625;
                const AlphaBound bnd = narrow ? alpha_bound_ends(cam, sa, ca, sb, cb, S.rsub[sub][0], S.rsub[sub][1])
                                              : alpha_bound(cam, rng);
                hi = bnd.hi;
                if (bnd.lo > 0.0f && tile_inside(cam, qx0, qx1, sy0, sy1))
                    atomicMax(&S.low2[sub * 4 + q], __float_as_int(bnd.lo));
            }
            S.hi2[sub * 4 + q][j] = hi;
        }
        __syncthreads();
        if (tid < OW_NQ) {
            const int sub = tid >> 2, q = tid & 3, nc = S.ncand[sub];
            const int sy0 = by0 + OW_Q * sub, sy1 = min(sy0 + OW_Q, H);
            const int qx0 = bx0 + OW_Q * q, qx1 = min(qx0 + OW_Q, bx1);
            int fill = OW_EVAL, qn = -1;
            if (sy0 >= H || qx0 >= bx1 || nc == 0) {
                fill = OW_NOBODY;                    // (outside the tile's part of the mosaic: never stored)
            } else if (S.subfill[sub] >= 0) {
                fill = S.subfill[sub];
            } else if (nc <= OW_QLIST) {
                const float L = __int_as_float(S.low2[tid]);
                qn = 0;
                for (int j = 0; j < nc; ++j)
                    if (S.hi2[tid][j] >= L) S.qlist[tid][qn++] = s_keep[sub * NL + j];
                if (qn == 0) {
                    fill = OW_NOBODY;                // every survivor is masked on the whole quarter
                } else if (qn == 1 && L > 0.0f) {
                    // one survivor with a positive lower bound: unmasked, above every other camera
                    // and a candidate (the bound counted only inside its rectangle) on every pixel
                    const int pos = S.qlist[tid][0];
                    if (tile_inside(cam_at(pos), qx0, qx1, sy0, sy1)) fill = index_at(pos);
                }
            }
            S.qn[tid] = qn;
            S.qfill[tid] = fill;
        }
        __syncthreads();
    }
    // ---- the quarters that need their pixels evaluated ---------------------------------------------
    if (wave == 0) {
        static_assert(OW_NQ <= 64, "one ballot lists the quarters to evaluate");
        const bool e = lane < OW_NQ && S.qfill[lane] == OW_EVAL && by0 + OW_Q * (lane >> 2) < H &&
                       bx0 + OW_Q * (lane & 3) < bx1;
        const unsigned long long bal = __ballot(e);
        if (e) S.evalq[__popcll(bal & ((1ull << lane) - 1ull))] = lane;
        if (lane == 0) S.n_eval = __popcll(bal);
    }
    __syncthreads();
    // an item = 16 columns x 4 OW_ILP rows of a quarter: lane -> column lane & 15, rows
    // (lane >> 4) + 4 j of the item's rows, OW_ILP independent pixels in flight per lane
    constexpr int PER_Q = 4 / OW_ILP;
    const int n_items = PER_Q * S.n_eval;
#pragma unroll 1
    for (int item = wave; item < n_items; item += 4) {
        const int qid = S.evalq[item / PER_Q], sub = qid >> 2, q = qid & 3;
        const int col = OW_Q * q + (lane & (OW_Q - 1));
        const int row0 = OW_Q * sub + 4 * OW_ILP * (item % PER_Q) + (lane >> 4);
        const int xc = min(bx0 + col, bx1 - 1);
        const double s = S.sn[col], c = S.cs[col];
        double t[OW_ILP];
        int y[OW_ILP], who[OW_ILP];
        float best[OW_ILP];
        bool any[OW_ILP];
#pragma unroll
        for (int j = 0; j < OW_ILP; ++j) {
            t[j] = S.tn[row0 + 4 * j];
            y[j] = min(by0 + row0 + 4 * j, by1 - 1);
            best[j] = 0.0f;
            who[j] = -1;
            any[j] = false;
        }
        const int mode = S.qn[qid];
        const int ncand = mode >= 0 ? mode : (mode == -1 ? S.ncand[sub] : (listed < 0 ? n : listed));
        for (int k = 0; k < ncand; ++k) {
            const int pos = __builtin_amdgcn_readfirstlane(
                mode >= 0 ? (int)S.qlist[qid][k] : (mode == -1 ? (int)s_keep[sub * NL + k] : k));
            const pano_camera *cam = cam_at(pos);
            const int i = index_at(pos);
            const int px = xc - cam->x0, sw = cam->sw, sh_ = cam->sh;
            const int cam_y0 = cam->y0, cam_h = cam->h;
            const bool in_x = (unsigned)px < (unsigned)cam->w;
            // The OW_ILP pixels in three passes - maps and taps, the hat tables' loads, alphas - and
            // every test as arithmetic (& not &&: a short-circuit put each pixel into a basic block
            // of its own, its loads waited for before the next pixel's map had begun): masked
            // pixels run the arithmetic too, on the taps of (0, 0).
            Taps tp[OW_ILP];
            bool ok[OW_ILP];
#pragma unroll
            for (int j = 0; j < OW_ILP; ++j) {
                float fx, fy;
                const bool m = map_pixel(cam->proj, s, c, t[j], sw, sh_, fx, fy);
                ok[j] = in_x & ((unsigned)(y[j] - cam_y0) < (unsigned)cam_h) & !m;
                tp[j] = make_taps_unmasked(ok[j] ? fx : 0.0f, ok[j] ? fy : 0.0f, sw, sh_);
            }
            typedef const __attribute__((address_space(1))) double *hat_ptr;
            const hat_ptr hat_x = (hat_ptr)cam->hat_x, hat_y = (hat_ptr)cam->hat_y;
            double hx0[OW_ILP], hx1[OW_ILP], hy0[OW_ILP], hy1[OW_ILP];
#pragma unroll
            for (int j = 0; j < OW_ILP; ++j) {
                hy0[j] = hat_y[tp[j].y0];
                hy1[j] = hat_y[tp[j].y1];
                hx0[j] = hat_x[tp[j].x0];
                hx1[j] = hat_x[tp[j].x1];
            }
#pragma unroll
            for (int j = 0; j < OW_ILP; ++j) {
                // alpha_at's arithmetic (geom.h): float32(hat_y * hat_x) per tap, the four taps' sum
                const float a = lerp4((float)(hy0[j] * hx0[j]), (float)(hy0[j] * hx1[j]),
                                      (float)(hy1[j] * hx0[j]), (float)(hy1[j] * hx1[j]), tp[j]);
                any[j] |= ok[j];
                const bool wins = ok[j] & (a > best[j]);     // strict: the first maximum keeps the pixel
                best[j] = wins ? a : best[j];
                who[j] = wins ? i : who[j];
            }
        }
#pragma unroll
        for (int j = 0; j < OW_ILP; ++j)
            S.town[row0 + 4 * j][col] = (short)(who[j] >= 0 ? who[j] : (any[j] ? OW_UNOWNED : OW_NOBODY));
    }
    __syncthreads();
    // ---- the tile leaves in 16-byte pieces: a lane takes eight pixels of a row, a wave eight rows per
    // store (a row per store - 64 two-byte and 64 one-byte lanes - was 64 stores a wave and, with the
    // run tracking in the same loop, a quarter of the workgroup's life: profiles/r05/own_stamps_*.txt)
    const int rows = by1 - by0, ncols = min(bx1 - bx0, OW_T);
    typedef short short8 __attribute__((ext_vector_type(8)));
    typedef short8 short8_any __attribute__((aligned(2)));       // a mosaic row starts anywhere
    typedef unsigned int uint2v __attribute__((ext_vector_type(2)));
    typedef uint2v uint2_any __attribute__((aligned(1)));
#pragma unroll
    for (int k = 0; k < OW_TH / 32; ++k) {
        const int row = 32 * k + 8 * wave + (lane >> 3), c0 = 8 * (lane & 7);
        if (row >= rows || c0 >= ncols) continue;
        const int fill = S.qfill[(row >> 4) * 4 + (c0 >> 4)];
        short8 w8 = (short)fill;
        if (fill == OW_EVAL) w8 = *(const short8 *)&S.town[row][c0];
        short8 own8;
        unsigned char ok8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int w = w8[j];
            own8[j] = (short)(w < 0 ? -1 : w);
            ok8[j] = (w >= 0 || w == OW_UNOWNED) ? 1 : 0;
        }
        const size_t g = (size_t)(by0 + row) * W + bx0 + c0;
        if (c0 + 8 <= ncols) {
            *(short8_any *)(owner + g) = own8;
            uint2v v;
            v.x = ok8[0] | ok8[1] << 8 | ok8[2] << 16 | (unsigned)ok8[3] << 24;
            v.y = ok8[4] | ok8[5] << 8 | ok8[6] << 16 | (unsigned)ok8[7] << 24;
            *(uint2_any *)(valid + g) = v;
        } else {
            for (int j = 0; j < ncols - c0; ++j) {
                owner[g + j] = own8[j];
                valid[g + j] = ok8[j];
            }
        }
    }
    if (!marks) return;
    // ---- boxes and column marks: a run of one owner down a column, per 16-row sub-tile; a quarter with
    // one owner (most of them) is one run without a look at its pixels
    const int x = bx0 + lane;
    const bool in_strip = x < bx1;
    auto flush = [&](int run_o, int run_y0, int run_y1) {
        if (run_o < 0 || !in_strip) return;
        marks[(size_t)run_o * W + x] = 1;
        if (n <= OWN_LIST) {
            int *b = s_box[run_o];
            atomicMin(&b[0], run_y0);
            atomicMax(&b[1], run_y1);
            atomicMin(&b[2], x);
            atomicMax(&b[3], x);
        } else {                             // more cameras than the LDS boxes hold: straight to memory
            box_merge(boxes + (size_t)box_stride * run_o, run_y0, run_y1, x, x);
        }
    };
#pragma unroll 1
    for (int sub = wave; sub < OW_SUBS; sub += 4) {
        const int r0 = OW_Q * sub, r1 = min(r0 + OW_Q, rows);
        if (r0 >= rows) break;
        const int fill = S.qfill[sub * 4 + (lane >> 4)];
        if (fill != OW_EVAL) {
            if (fill >= 0 && in_strip) {
                // the quarter's 16 columns: every lane marks its column, the first one merges the box
                marks[(size_t)fill * W + x] = 1;
                if ((lane & 15) == 0) {
                    const int x1 = min(x + OW_Q, bx1) - 1;
                    if (n <= OWN_LIST) {
                        int *b = s_box[fill];
                        atomicMin(&b[0], by0 + r0);
                        atomicMax(&b[1], by0 + r1 - 1);
                        atomicMin(&b[2], x);
                        atomicMax(&b[3], x1);
                    } else {
                        box_merge(boxes + (size_t)box_stride * fill, by0 + r0, by0 + r1 - 1, x, x1);
                    }
                }
            }
        } else {
            int run_o = -1, run_y0 = 0, run_y1 = 0;
            for (int row = r0; row < r1; ++row) {
                const int t = S.town[row][lane], w = t < 0 ? -1 : t;
                const int y = by0 + row;
                if (w != run_o) {
                    flush(run_o, run_y0, run_y1);
                    run_o = w;
                    run_y0 = y;
                }
                run_y1 = y;
            }
            flush(run_o, run_y0, run_y1);
        }
    }
    __syncthreads();
    if (n <= OWN_LIST && tid < n) {
        const int *b = s_box[tid];
        if (b[1] >= b[0]) box_merge(boxes + (size_t)box_stride * tid, b[0], b[1], b[2], b[3]);
    }
}

__global__ __launch_bounds__(256) void OW_FN(ownership_cameras_kernel)(
    const pano_camera *__restrict__ cams, int n, int H, int W, int xs0, int xs1,
    const double *__restrict__ sin_t, const double *__restrict__ cos_t,
    const double *__restrict__ tan_p, int16_t *__restrict__ owner,
    uint8_t *__restrict__ valid, int prune, int32_t *__restrict__ boxes, int box_stride,
    uint8_t *__restrict__ marks) {
    extern __shared__ __align__(16) unsigned char own_smem[];
    OW_FN(OwnShared) &S = *(OW_FN(OwnShared) *)own_smem;
    const int NL = min(n, OWN_LIST);
    int (*s_box)[4] = (int (*)[4])(own_smem + ((sizeof(OW_FN(OwnShared)) + 15) & ~(size_t)15));
    float *s_hi = (float *)(s_box + NL);
    short *s_keep = (short *)(s_hi + OW_SUBS * NL);
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    const int bx0 = xs0 + blockIdx.x * OW_T, by0 = blockIdx.y * OW_TH;
    const int bx1 = min(bx0 + OW_T, xs1), by1 = min(by0 + OW_TH, H);
    // (a workgroup's wave w sits on SIMD w: the few threads of the bound passes rotate with the
    // workgroup so that they do not all queue on SIMD 0)
    const int vt = (tid + 64 * (int)((blockIdx.x + blockIdx.y) & 3)) & 255;
    if (marks && tid < NL) {
        int *b = s_box[tid];
        b[0] = b[2] = 0x7fffffff;
        b[1] = b[3] = -1;
    }
    // Everything the tile reads from memory leaves now, together with the rectangles the list is
    // built from: the tile's trigonometry (wave 0 the columns, wave 1 the rows) and, when there
    // are few cameras, all their records (pano_camera = 30 dwords; else the listed ones follow)
    constexpr int DW = (int)(sizeof(pano_camera) / 4);
    const bool all_cams = n <= OW_CAMS;
    uint32_t rec_dw[(OW_CAMS * DW + 255) / 256];
    if (all_cams) {
#pragma unroll
        for (int r = 0; r < (OW_CAMS * DW + 255) / 256; ++r) {
            const int d = tid + 256 * r;
            rec_dw[r] = d < n * DW ? ((const uint32_t *)cams)[d] : 0u;
        }
    }
    double tv = 0.0, tw = 0.0;
    if (wave == 0) {
        const int xc = min(bx0 + lane, bx1 - 1);
        tv = table_f64(sin_t, xc);
        tw = table_f64(cos_t, xc);
    }
    double trow[OW_TH / 64 > 0 ? OW_TH / 64 : 1];
    if (wave == 1) {
#pragma unroll
        for (int r = 0; r < OW_TH / 64; ++r) trow[r] = table_f64(tan_p, min(by0 + 64 * r + lane, by1 - 1));
    }
    const int listed = build_camera_list(S.cl, cams, n, bx0, bx1, by0, by1);
    const int mode = all_cams ? 2 : (listed >= 0 && listed <= OW_CAMS ? 1 : 0);
    uint32_t *dst = (uint32_t *)S.cam;
    if (all_cams) {
#pragma unroll
        for (int r = 0; r < (OW_CAMS * DW + 255) / 256; ++r) {
            const int d = tid + 256 * r;
            if (d < n * DW) dst[d] = rec_dw[r];
        }
    } else if (mode == 1) {
        for (int d = tid; d < listed * DW; d += 256) {
            const int rec = d / DW, w = d - rec * DW;
            dst[d] = ((const uint32_t *)(cams + S.cl.list[rec]))[w];
        }
    }
    if (wave == 0) {
        S.sn[lane] = tv;
        S.cs[lane] = tw;
        double lo_s = tv, hi_s = tv, lo_c = tw, hi_c = tw;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            lo_s = fmin(lo_s, __shfl_xor(lo_s, off, 64));
            hi_s = fmax(hi_s, __shfl_xor(hi_s, off, 64));
            lo_c = fmin(lo_c, __shfl_xor(lo_c, off, 64));
            hi_c = fmax(hi_c, __shfl_xor(hi_c, off, 64));
            if (off == OW_Q / 2 && (lane & (OW_Q - 1)) == 0) {
                double *r = S.rq[lane / OW_Q];
                r[0] = lo_s, r[1] = hi_s, r[2] = lo_c, r[3] = hi_c;
            }
        }
        if (lane == 0) S.rall[0] = lo_s, S.rall[1] = hi_s, S.rall[2] = lo_c, S.rall[3] = hi_c;
        // the columns' angles are equally spaced: the angle a run of k columns spans is k times the
        // step, whose chord the first two columns give (a tile of one column spans nothing); the
        // end columns' form of the bound is used for runs below a quarter of a radian - the chord
        // of the END columns alone would also be short for a run that wraps around the circle
        const double s1 = __shfl(tv, 1, 64), c1 = __shfl(tw, 1, 64);
        if (lane == 0) S.step2 = bx1 - bx0 >= 2 ? (s1 - tv) * (s1 - tv) + (c1 - tw) * (c1 - tw) : 0.0;
    } else if (wave == 1) {
        static_assert(OW_TH % 64 == 0, "whole waves of rows");
#pragma unroll
        for (int r = 0; r < OW_TH / 64; ++r) {
            S.tn[64 * r + lane] = trow[r];
            double lo_t = trow[r], hi_t = trow[r];
#pragma unroll
            for (int off = 1; off < OW_Q; off <<= 1) {
                lo_t = fmin(lo_t, __shfl_xor(lo_t, off, 64));
                hi_t = fmax(hi_t, __shfl_xor(hi_t, off, 64));
            }
            if ((lane & (OW_Q - 1)) == 0)
                S.rsub[4 * r + lane / OW_Q][0] = lo_t, S.rsub[4 * r + lane / OW_Q][1] = hi_t;
        }
    } else if (wave == 2 && lane < OW_NQ) {
        S.low2[lane] = 0;
        S.qn[lane] = -2;
        S.qfill[lane] = OW_EVAL;
        if (lane < OW_SUBS) S.low1[lane] = 0, S.ncand[lane] = 0;
    }
    __syncthreads();
#define OW_CALL(M)                                                                                  \
    OW_FN(own_tile)<M>(S, s_box, s_hi, s_keep, NL, cams, n, H, W, bx0, bx1, by0, by1, listed, prune, vt,  \
                owner, valid, boxes, box_stride, marks)
    if (mode == 2)
        OW_CALL(2);
    else if (mode == 1)
        OW_CALL(1);
    else
        OW_CALL(0);
#undef OW_CALL
}


#undef OW_TH
#undef OW_NQ
