/* Test restatement of CV_HAAR_FIND_BIGGEST_OBJECT (cvHaarDetectObjects' flags bit 2, tempcv.hpp:129; with CV_HAAR_DO_ROUGH_SEARCH,
 * bit 3) on top of the CPU oracle — tempcv.cpp:1188-1503 with findBiggestObject set:
 *   the flags CV_HAAR_SCALE_IMAGE and CV_HAAR_DO_CANNY_PRUNING are cleared            :1227, :1254
 *   n_factors counted upwards, the factors walked down by the reciprocal                :1344-1361
 *   per scale: ystep, winSize, the break on minSize, the ranges of a scanROI            :1365-1415
 *   the walk of the rows (ixstep = result != 0 ? 1 : 2 from startX of every row)        :1132-1175
 *   after a scale: group, maxRect, push it, scanROI, minSize                            :1422-1454
 *   at the end: group everything, the first group of strictly greatest area            :1458-1490
 * The window evaluation is the oracle's (cvSetImagesForHaarClassifierCascade at the scale's factor, cvRunHaarClassifierCascadeSum
 * with the border rule: detect_opencvlike_impl's arithmetic, statement for statement, as a function of (factor, x, y)), the
 * grouping is oc_group_rectangles.  Built by tests/find_biggest_oracle.py with oracle/Makefile's flags; oracle/ is not modified. */
#include "../oracle/vj_oracle.c"

#include <float.h>

typedef struct fb_setup {
    cv_node* kn;
    int q0, q1, q2, q3;
    double weight_scale;
    int is_stump_based, is_tree, has_tilted;
    int two_rects[64];
} fb_setup;

static void fb_flags(const oc_cascade* c, fb_setup* s) {   /* icvCreateHidHaarClassifierCascade (:410-470) */
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

/* cvSetImagesForHaarClassifierCascade(cascade, sum, sqsum, tilted, factor) (:549-768) for a sum image of row length sw */
static void fb_set_images(const oc_cascade* c, int sw, double factor, fb_setup* s) {
    const int ex = cv_round(factor), ew = cv_round((c->win_w - 2) * factor), eh = cv_round((c->win_h - 2) * factor);
    s->weight_scale = 1. / (ew * eh);
    s->q0 = ex * sw + ex;
    s->q1 = ex * sw + ex + ew;
    s->q2 = (ex + eh) * sw + ex;
    s->q3 = (ex + eh) * sw + ex + ew;
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
            const int tx = cv_round(r[0] * factor), ty = cv_round(r[1] * factor);
            const int tw = cv_round(r[2] * factor), th = cv_round(r[3] * factor);
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

/* cvRunHaarClassifierCascade at (x, y) for a window of win_w x win_h: > 0 pass, 0 or -i reject, -1 at the border (:817-820) */
static int fb_run(const oc_cascade* c, const fb_setup* s, const int32_t* sum, const double* sqsum, const int32_t* tilted, int sw, int sh,
                  int win_w, int win_h, int x, int y, oc_stats* st) {
    if (x < 0 || y < 0 || x + win_w >= sw || y + win_h >= sh) return -1;
    const cv_node* kn = s->kn;
    const int po = y * sw + x;
    const double mean = (double)(int)((uint32_t)sum[po + s->q0] - (uint32_t)sum[po + s->q1] - (uint32_t)sum[po + s->q2] + (uint32_t)sum[po + s->q3]) *
                        s->weight_scale;
    double vnf = sqsum[po + s->q0] - sqsum[po + s->q1] - sqsum[po + s->q2] + sqsum[po + s->q3];
    vnf = vnf * s->weight_scale - mean * mean;
    vnf = vnf >= 0. ? sqrt(vnf) : 1.;
    if (s->is_tree) {   /* :834-861: any reject returns 0 */
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
                if (s->two_rects[i]) {   /* :872-888 */
                    const int32_t* img = k->tilted ? tilted : sum;
                    double rect0 = cv_calc_sum(img, po, &k->rect[0]);
                    rect0 *= k->rect[0].weight;
                    double rect1 = cv_calc_sum(img, po, &k->rect[1]);
                    rect1 *= k->rect[1].weight;
                    v = rect1 + rect0;
                } else {                 /* :907-911 */
                    v = cv_node_sum_f32(sum, tilted, po, k);
                }
                stage_sum += alpha[v >= tt];
            } else {                     /* :952-957 */
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

/* What the search did, for inspection */
typedef struct fb_info {
    int32_t found;              /* 1: `result` is valid */
    int32_t result[4];          /* x y w h */
    int32_t neighbors;
    int32_t n_factors;
    int32_t scales_evaluated;   /* iterations that reached the walk (the break on minSize ends them) */
    int32_t first_hit_scale;    /* scale_idx of the iteration after which maxRect was found, -1: never */
    int32_t roi_scales;         /* iterations walked inside the scanROI */
    int32_t roi_candidates;     /* candidates found there */
    int32_t roi[4];             /* scanROI, as clamped */
    int32_t roi_clamped;        /* 1: one of the four clamps of :1445-1448 changed a value */
    int32_t min_size[2];        /* minSize after the hit */
} fb_info;

/* cand (may be NULL): up to cap candidates in allCandidates' order, scale_idx = n_factors - 1 - k of the iteration, and -2 for the
 * pushed maxRect; *n_total counts them all.  Returns the number written. */
int fb_detect_biggest(const oc_cascade* c, const uint8_t* gray, int W, int H, int stride, int min_w, int min_h, double scaleFactor,
                      int minNeighbors, int roughSearch, oc_rect* cand, int cap, int* n_total, oc_stats* st, fb_info* info) {
    const double GROUP_EPS = 0.2;
    const int sw = W + 1, sh = H + 1;
    int32_t* sum = (int32_t*)calloc((size_t)sw * (H + 3), sizeof(int32_t));
    double* sqsum = (double*)calloc((size_t)sw * (H + 3), sizeof(double));
    int32_t* tilted = NULL;
    fb_setup s;
    memset(st, 0, sizeof(*st));
    memset(info, 0, sizeof(*info));
    info->first_hit_scale = -1;
    s.kn = (cv_node*)malloc(sizeof(cv_node) * (size_t)c->n_nodes);
    fb_flags(c, &s);
    oc_integral(gray, W, H, stride, sum, sqsum);
    if (s.has_tilted) {
        tilted = (int32_t*)calloc((size_t)sw * (H + 3), sizeof(int32_t));
        oc_integral_tilted(gray, W, H, stride, tilted);
    }
    int all_cap = 1024, n_all = 0;
    oc_rect* all = (oc_rect*)malloc(sizeof(oc_rect) * (size_t)all_cap);
#define FB_PUSH(X, Y, Wd, Ht, IDX)                                                        \
    do {                                                                                  \
        if (n_all == all_cap) all = (oc_rect*)realloc(all, sizeof(oc_rect) * (size_t)(all_cap *= 2)); \
        all[n_all].x = (X); all[n_all].y = (Y); all[n_all].w = (Wd); all[n_all].h = (Ht); all[n_all].scale_idx = (IDX); \
        ++n_all;                                                                          \
    } while (0)
    int n_factors = 0;
    double factor;
    for (n_factors = 0, factor = 1; factor * c->win_w < W - 10 && factor * c->win_h < H - 10; n_factors++, factor *= scaleFactor) {}
    info->n_factors = n_factors;
    scaleFactor = 1. / scaleFactor;
    factor *= scaleFactor;
    int roi_x = 0, roi_y = 0, roi_w = 0, roi_h = 0;   /* scanROI */
    int left = n_factors, k = 0;
    for (; left-- > 0; factor *= scaleFactor, ++k) {
        const double ystep = 2. > factor ? 2. : factor;
        const int win_w = cv_round(c->win_w * factor), win_h = cv_round(c->win_h * factor);
        int startX = 0, startY = 0;
        int endX = cv_round((W - win_w) / ystep), endY = cv_round((H - win_h) / ystep);
        if (win_w < min_w || win_h < min_h) break;
        fb_set_images(c, sw, factor, &s);
        const int in_roi = roi_w * roi_h > 0;
        if (in_roi) {
            startY = cv_round(roi_y / ystep);
            endY = cv_round((roi_y + roi_h - win_h) / ystep);
            startX = cv_round(roi_x / ystep);
            endX = cv_round((roi_x + roi_w - win_w) / ystep);
            info->roi_scales++;
        }
        info->scales_evaluated++;
        for (int iy = startY; iy < endY; iy++) {
            const int y = cv_round(iy * ystep);
            int ixstep = 1;
            for (int ix = startX; ix < endX; ix += ixstep) {
                const int x = cv_round(ix * ystep);
                st->windows++;
                const int result = fb_run(c, &s, sum, sqsum, tilted, sw, sh, win_w, win_h, x, y, st);
                if (result > 0) {
                    FB_PUSH(x, y, win_w, win_h, n_factors - 1 - k);
                    if (in_roi) info->roi_candidates++;
                }
                ixstep = result != 0 ? 1 : 2;
            }
        }
        if (n_all != 0 && roi_w * roi_h == 0) {
            oc_grect* list = (oc_grect*)malloc(sizeof(oc_grect) * (size_t)n_all);
            int32_t* weights = (int32_t*)malloc(sizeof(int32_t) * (size_t)n_all);
            for (int i = 0; i < n_all; ++i) { list[i].x = all[i].x; list[i].y = all[i].y; list[i].w = all[i].w; list[i].h = all[i].h; }
            const int n = oc_group_rectangles(list, n_all, minNeighbors > 1 ? minNeighbors : 1, GROUP_EPS, weights);
            if (n != 0) {
                oc_grect maxRect = {0, 0, 0, 0};
                for (int i = 0; i < n; ++i)
                    if (list[i].w * list[i].h > maxRect.w * maxRect.h) maxRect = list[i];
                FB_PUSH(maxRect.x, maxRect.y, maxRect.w, maxRect.h, -2);
                const int dx = cv_round(maxRect.w * GROUP_EPS), dy = cv_round(maxRect.h * GROUP_EPS);
                roi_x = maxRect.x - dx > 0 ? maxRect.x - dx : 0;
                roi_y = maxRect.y - dy > 0 ? maxRect.y - dy : 0;
                roi_w = maxRect.w + dx * 2 < W - 1 - roi_x ? maxRect.w + dx * 2 : W - 1 - roi_x;
                roi_h = maxRect.h + dy * 2 < H - 1 - roi_y ? maxRect.h + dy * 2 : H - 1 - roi_y;
                info->roi_clamped = maxRect.x - dx < 0 || maxRect.y - dy < 0 || roi_w != maxRect.w + dx * 2 || roi_h != maxRect.h + dy * 2;
                const double minScale = roughSearch ? 0.6 : 0.4;
                min_w = cv_round(maxRect.w * minScale);
                min_h = cv_round(maxRect.h * minScale);
                info->first_hit_scale = n_factors - 1 - k;
                info->roi[0] = roi_x; info->roi[1] = roi_y; info->roi[2] = roi_w; info->roi[3] = roi_h;
                info->min_size[0] = min_w; info->min_size[1] = min_h;
            }
            free(list); free(weights);
        }
    }
    /* :1458-1490 */
    if (n_all != 0) {
        oc_grect* list = (oc_grect*)malloc(sizeof(oc_grect) * (size_t)n_all);
        int32_t* weights = (int32_t*)malloc(sizeof(int32_t) * (size_t)n_all);
        for (int i = 0; i < n_all; ++i) { list[i].x = all[i].x; list[i].y = all[i].y; list[i].w = all[i].w; list[i].h = all[i].h; }
        const int n = oc_group_rectangles(list, n_all, minNeighbors > 1 ? minNeighbors : 1, GROUP_EPS, weights);
        int area = 0;
        for (int i = 0; i < n; ++i)
            if (list[i].w * list[i].h > area) {
                area = list[i].w * list[i].h;
                info->found = 1;
                info->result[0] = list[i].x; info->result[1] = list[i].y; info->result[2] = list[i].w; info->result[3] = list[i].h;
                info->neighbors = weights[i];
            }
        free(list); free(weights);
    }
    int written = 0;
    for (int i = 0; i < n_all && cand && i < cap; ++i) cand[written++] = all[i];
    *n_total = n_all;
#undef FB_PUSH
    free(all); free(s.kn); free(sum); free(sqsum); free(tilted);
    return written;
}
