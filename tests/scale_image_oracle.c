/* Test restatement of CV_HAAR_SCALE_IMAGE (cvHaarDetectObjects' flags bit 1, tempcv.hpp:128; tempcv.cpp:1257-1329 and the invoker
 * :989-1113) on top of the CPU oracle:
 *   si_resize_linear        cvResize(src, dst, CV_INTER_LINEAR) for 8-bit single-channel images as DESIGN.md §4.8 states it (OpenCV
 *                           2.4.2 imgproc: third-party, parity unpinned), pixel by pixel straight from the formulas — no coefficient
 *                           tables (the device builds tables on the host and applies them in a kernel)
 *   si_level_verdicts       cvRunHaarClassifierCascadeSum at every grid position of ONE image with the cascade set up at scale 1.
 *                           (cvSetImagesForHaarClassifierCascade(.., 1.)): the oracle's detect_opencvlike_impl arithmetic restated
 *                           at factor 1 (the anchor test compares it with that walk on a frame that has a single factor)
 *   si_detect_scale_image   the level loop: resize, oc_integral / oc_integral_tilted per level, every position, no skip
 * Built by tests/scale_image_oracle.py with oracle/Makefile's flags.  oracle/ itself is not modified.                      */
#include "../oracle/vj_oracle.c"

#include <float.h>

static void si_src_coord(int d, double scale, int* i, float* f) {
    *f = (float)((d + 0.5) * scale - 0.5);
    *i = (int)floorf(*f);
    *f -= (float)*i;
}
static inline int si_coef(float v) {   /* saturate_cast<short>(v * 2048): cvRound, half to even */
    int r = cv_round((double)(v * 2048.f));
    return r < -32768 ? -32768 : r > 32767 ? 32767 : r;
}
static inline int si_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

void si_resize_linear(const uint8_t* src, int sw, int sh, int sstride, uint8_t* dst, int dw, int dh, int dstride) {
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    if (fabs(scale_x - 2.) < DBL_EPSILON && fabs(scale_y - 2.) < DBL_EPSILON) {   /* OpenCV's area path for exactly 2:1 */
        for (int y = 0; y < dh; ++y)
            for (int x = 0; x < dw; ++x) {
                const uint8_t* a = src + (size_t)(2 * y) * sstride + 2 * x;
                const uint8_t* b = src + (size_t)(2 * y + 1) * sstride + 2 * x;
                dst[(size_t)y * dstride + x] = (uint8_t)((a[0] + a[1] + b[0] + b[1] + 2) >> 2);
            }
        return;
    }
    for (int y = 0; y < dh; ++y) {
        int sy;
        float fy;
        si_src_coord(y, scale_y, &sy, &fy);   /* the fraction stays; the two ROW INDICES are clamped */
        const uint8_t* r0 = src + (size_t)si_clampi(sy, 0, sh - 1) * sstride;
        const uint8_t* r1 = src + (size_t)si_clampi(sy + 1, 0, sh - 1) * sstride;
        const int b0 = si_coef(1.f - fy), b1 = si_coef(fy);
        for (int x = 0; x < dw; ++x) {
            int sx;
            float fx;
            si_src_coord(x, scale_x, &sx, &fx);
            if (sx < 0) { sx = 0; fx = 0.f; }
            int h0, h1;
            if (sx >= sw - 1) {                 /* past the last column: one tap */
                sx = sw - 1;
                h0 = r0[sx] * 2048;
                h1 = r1[sx] * 2048;
            } else {
                const int a0 = si_coef(1.f - fx), a1 = si_coef(fx);
                h0 = r0[sx] * a0 + r0[sx + 1] * a1;
                h1 = r1[sx] * a0 + r1[sx + 1] * a1;
            }
            dst[(size_t)y * dstride + x] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
        }
    }
}

/* The cascade at scale 1. on an image of width w (cvSetImagesForHaarClassifierCascade, tempcv.cpp:549-768, with scale = 1.) */
typedef struct si_setup {
    cv_node* kn;
    int q0, q1, q2, q3;
    double weight_scale;
    int is_stump_based, is_tree, has_tilted;
    int two_rects[64];
} si_setup;

static void si_flags(const oc_cascade* c, si_setup* s) {   /* icvCreateHidHaarClassifierCascade (:410-470) */
    s->is_stump_based = 1;
    s->is_tree = 0;
    s->has_tilted = 0;
    for (int t = 0; t < c->n_trees; ++t) s->is_stump_based &= c->tree_n_nodes[t] == 1;
    for (int i = 0; i < c->n_stages && i < 64; ++i) {
        s->is_tree |= c->stage_next[i] != -1;
        s->two_rects[i] = 1;
        for (int t = c->stage_first_tree[i]; t < c->stage_first_tree[i] + c->stage_n_trees[i]; ++t)
            for (int l = 0; l < c->tree_n_nodes[t]; ++l) {
                const int n = c->tree_first_node[t] + l;
                const int32_t* r2 = c->node_rect + (n * 3 + 2) * 4;
                if (!(fabs((double)c->node_weight[n * 3 + 2]) < DBL_EPSILON || r2[2] == 0 || r2[3] == 0)) s->two_rects[i] = 0;
                if (c->node_tilted && c->node_tilted[n]) s->has_tilted = 1;
            }
    }
}

static void si_set_images(const oc_cascade* c, int w, si_setup* s) {
    const int sw = w + 1;
    const int ew = c->win_w - 2, eh = c->win_h - 2;   /* equ_rect = (1, 1, win_w - 2, win_h - 2) */
    s->weight_scale = 1. / (ew * eh);
    s->q0 = sw + 1;
    s->q1 = sw + 1 + ew;
    s->q2 = (1 + eh) * sw + 1;
    s->q3 = (1 + eh) * sw + 1 + ew;
    for (int n = 0; n < c->n_nodes; ++n) {
        cv_node* k = s->kn + n;
        const int32_t* r2 = c->node_rect + (n * 3 + 2) * 4;
        double sum0 = 0, area0 = 0;
        k->nrect = (fabs((double)c->node_weight[n * 3 + 2]) < DBL_EPSILON || r2[2] == 0 || r2[3] == 0) ? 2 : 3;
        k->tilted = c->node_tilted ? c->node_tilted[n] != 0 : 0;
        k->threshold = c->node_threshold[n];
        const double correction_ratio = s->weight_scale * (!k->tilted ? 1 : 0.5);
        for (int j = 0; j < k->nrect; ++j) {
            const int32_t* r = c->node_rect + (n * 3 + j) * 4;
            const int tx = r[0], ty = r[1], tw = r[2], th = r[3];   /* cvRound(v * 1.) = v */
            if (!k->tilted) {
                k->rect[j].p0 = ty * sw + tx;
                k->rect[j].p1 = ty * sw + tx + tw;
                k->rect[j].p2 = (ty + th) * sw + tx;
                k->rect[j].p3 = (ty + th) * sw + tx + tw;
            } else {
                k->rect[j].p2 = (ty + tw) * sw + tx + tw;
                k->rect[j].p3 = (ty + tw + th) * sw + tx + tw - th;
                k->rect[j].p0 = ty * sw + tx;
                k->rect[j].p1 = (ty + th) * sw + tx - th;
            }
            k->rect[j].weight = (float)(c->node_weight[n * 3 + j] * correction_ratio);
            if (j == 0) area0 = tw * th;
            else sum0 += k->rect[j].weight * tw * th;
        }
        k->rect[0].weight = (float)(-sum0 / area0);
    }
}

/* cvRunHaarClassifierCascadeSum at (x, y): > 0 pass, 0 or -i reject */
static int si_run(const oc_cascade* c, const si_setup* s, const int32_t* sum, const double* sqsum, const int32_t* tilted, int sw, int x, int y,
                  oc_stats* st) {
    const cv_node* kn = s->kn;
    const int po = y * sw + x;
    const double mean = (double)(int)((uint32_t)sum[po + s->q0] - (uint32_t)sum[po + s->q1] - (uint32_t)sum[po + s->q2] + (uint32_t)sum[po + s->q3]) *
                        s->weight_scale;
    double vnf = sqsum[po + s->q0] - sqsum[po + s->q1] - sqsum[po + s->q2] + sqsum[po + s->q3];
    vnf = vnf * s->weight_scale - mean * mean;
    vnf = vnf >= 0. ? sqrt(vnf) : 1.;
    if (s->is_tree) {
        int ptr = 0;
        while (ptr != -1) {
            double stage_sum = 0.0;
            st->stage_entered[ptr]++;
            for (int t = c->stage_first_tree[ptr]; t < c->stage_first_tree[ptr] + c->stage_n_trees[ptr]; ++t) {
                const int n0 = c->tree_first_node[t];
                int idx = 0;
                do {
                    const cv_node* k = kn + n0 + idx;
                    st->stump_evals++;
                    idx = cv_node_sum_f32(sum, tilted, po, k) < k->threshold * vnf ? c->node_left[n0 + idx] : c->node_right[n0 + idx];
                } while (idx > 0);
                stage_sum += c->alpha[c->tree_first_alpha[t] - idx];
            }
            if (stage_sum >= c->stage_threshold[ptr] - 0.0001f) {
                ptr = c->stage_child[ptr];
            } else {
                while (ptr != -1 && c->stage_next[ptr] == -1) ptr = c->stage_parent[ptr];
                if (ptr == -1) return 0;
                ptr = c->stage_next[ptr];
            }
        }
        return 1;
    }
    for (int i = 0; i < c->n_stages; ++i) {
        double stage_sum = 0.0;
        st->stage_entered[i]++;
        for (int t = c->stage_first_tree[i]; t < c->stage_first_tree[i] + c->stage_n_trees[i]; ++t) {
            const int n0 = c->tree_first_node[t];
            const float* alpha = c->alpha + c->tree_first_alpha[t];
            if (s->is_stump_based) {
                const cv_node* k = kn + n0;
                const double tt = k->threshold * vnf;
                double v;
                st->stump_evals++;
                if (s->two_rects[i]) {
                    const int32_t* img = k->tilted ? tilted : sum;
                    double rect0 = cv_calc_sum(img, po, &k->rect[0]);
                    rect0 *= k->rect[0].weight;
                    double rect1 = cv_calc_sum(img, po, &k->rect[1]);
                    rect1 *= k->rect[1].weight;
                    v = rect1 + rect0;
                } else {
                    v = cv_node_sum_f32(sum, tilted, po, k);
                }
                stage_sum += alpha[v >= tt];
            } else {
                int idx = 0;
                do {
                    const cv_node* k = kn + n0 + idx;
                    st->stump_evals++;
                    idx = cv_node_sum_f32(sum, tilted, po, k) < k->threshold * vnf ? c->node_left[n0 + idx] : c->node_right[n0 + idx];
                } while (idx > 0);
                stage_sum += alpha[-idx];
            }
        }
        if (stage_sum < c->stage_threshold[i] - 0.0001f) return -i;
    }
    return 1;
}

/* One level: the integrals of `img` (w x h) and the verdict of every grid position x, y = 0, ystep, ... < size - window.
 * verdicts (may be NULL): ny x nx ints, row-major.  Returns the number of positions. */
static long si_level(const oc_cascade* c, si_setup* s, const uint8_t* img, int w, int h, int stride, int ystep, int* verdicts, oc_stats* st,
                     double factor, int win_w, int win_h, int scale_idx, oc_rect* out, int cap, int* found) {
    const int sw = w + 1;
    int32_t* sum = (int32_t*)calloc((size_t)sw * (h + 1), sizeof(int32_t));
    double* sqsum = (double*)calloc((size_t)sw * (h + 1), sizeof(double));
    int32_t* tilted = NULL;
    oc_integral(img, w, h, stride, sum, sqsum);
    if (s->has_tilted) {
        tilted = (int32_t*)calloc((size_t)sw * (h + 1), sizeof(int32_t));
        oc_integral_tilted(img, w, h, stride, tilted);
    }
    si_set_images(c, w, s);
    long n = 0;
    for (int y = 0; y < h - c->win_h; y += ystep)
        for (int x = 0; x < w - c->win_w; x += ystep) {
            const int result = si_run(c, s, sum, sqsum, tilted, sw, x, y, st);
            st->windows++;
            if (verdicts) verdicts[n] = result;
            ++n;
            if (result > 0 && out) {
                if (*found < cap) {
                    out[*found].x = cv_round(x * factor);
                    out[*found].y = cv_round(y * factor);
                    out[*found].w = win_w;
                    out[*found].h = win_h;
                    out[*found].scale_idx = scale_idx;
                }
                ++*found;
            }
        }
    free(sum); free(sqsum); free(tilted);
    return n;
}

long si_level_verdicts(const oc_cascade* c, const uint8_t* gray, int W, int H, int stride, int ystep, int* verdicts, oc_stats* st) {
    si_setup s;
    memset(st, 0, sizeof(*st));
    s.kn = (cv_node*)malloc(sizeof(cv_node) * (size_t)c->n_nodes);
    si_flags(c, &s);
    const long n = si_level(c, &s, gray, W, H, stride, ystep, verdicts, st, 1., c->win_w, c->win_h, 0, NULL, 0, NULL);
    free(s.kn);
    return n;
}

/* level_sizes (may be NULL): up to 64 x {w, h} of the evaluated levels; *n_levels counts them all */
int si_detect_scale_image(const oc_cascade* c, const uint8_t* gray, int W, int H, int stride, int min_w, int min_h, double scaleFactor,
                          oc_rect* out, int cap, int* n_total, oc_stats* st, int* n_levels, int* level_sizes) {
    si_setup s;
    memset(st, 0, sizeof(*st));
    s.kn = (cv_node*)malloc(sizeof(cv_node) * (size_t)c->n_nodes);
    si_flags(c, &s);
    uint8_t* small = (uint8_t*)malloc((size_t)W * H);
    int found = 0, levels = 0, scale_idx = 0;
    for (double factor = 1;; factor *= scaleFactor, ++scale_idx) {
        const int win_w = cv_round(c->win_w * factor), win_h = cv_round(c->win_h * factor);
        const int sz_w = cv_round(W / factor), sz_h = cv_round(H / factor);
        if (sz_w - c->win_w + 1 <= 0 || sz_h - c->win_h + 1 <= 0) break;
        if (win_w > W || win_h > H) break;     /* maxSize = the image */
        if (win_w < min_w || win_h < min_h) continue;
        si_resize_linear(gray, W, H, stride, small, sz_w, sz_h, sz_w);
        si_level(c, &s, small, sz_w, sz_h, sz_w, factor > 2 ? 1 : 2, NULL, st, factor, win_w, win_h, scale_idx, out, cap, &found);
        if (level_sizes && levels < 64) { level_sizes[2 * levels] = sz_w; level_sizes[2 * levels + 1] = sz_h; }
        ++levels;
    }
    free(small); free(s.kn);
    *n_total = found;
    *n_levels = levels;
    return found < cap ? found : cap;
}
