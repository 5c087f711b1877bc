/* Test restatement of cvHaarDetectObjectsForROC with outputRejectLevels = true (tempcv.hpp:282-286; tempcv.cpp:1188-1503) on top
 * of tests/scale_image_oracle.c (the resize, the cascade at scale 1, the integrals) and oracle/vj_oracle.c (cv::partition):
 *   roc_run             cvRunHaarClassifierCascadeSum (:795-972) returning BOTH of its results: the int, and stage_sum, the
 *                       reference parameter that holds the sum of the last stage evaluated when the function returns
 *   roc_detect          the level loop with maxSize (:1230-1234, :1268-1288) and the ROC invoker's body (:1079-1095): a pass
 *                       becomes -count, a window is reported iff count + result < 4, with -result and stage_sum
 *   roc_group           groupRectangles' level overload (:255-258 -> :145-243), quirks included
 * Built by tests/roc_oracle.py with the flags of tests/scale_image_oracle.py.                                              */
#include "scale_image_oracle.c"

/* cvRunHaarClassifierCascadeSum at (x, y) with the cascade at scale 1 (no border rule can fire on the scale-image grid):
 * the return value, and *stage_sum as the caller finds it afterwards */
static int roc_run(const oc_cascade* c, const si_setup* s, const int32_t* sum, const double* sqsum, const int32_t* tilted, int sw, int x, int y,
                   double* stage_sum_out) {
    const cv_node* kn = s->kn;
    const int po = y * sw + x;
    const double mean = (double)(int)((uint32_t)sum[po + s->q0] - (uint32_t)sum[po + s->q1] - (uint32_t)sum[po + s->q2] + (uint32_t)sum[po + s->q3]) *
                        s->weight_scale;                                             /* :824-825 */
    double vnf = sqsum[po + s->q0] - sqsum[po + s->q1] - sqsum[po + s->q2] + sqsum[po + s->q3];
    vnf = vnf * s->weight_scale - mean * mean;                                       /* :826-832 */
    vnf = vnf >= 0. ? sqrt(vnf) : 1.;
    double stage_sum = 0.0;
    if (s->is_tree) {                                                                /* :834-861 */
        int ptr = 0;
        while (ptr != -1) {
            stage_sum = 0.0;
            for (int t = c->stage_first_tree[ptr]; t < c->stage_first_tree[ptr] + c->stage_n_trees[ptr]; ++t) {
                const int n0 = c->tree_first_node[t];
                int idx = 0;
                do {
                    const cv_node* k = kn + n0 + idx;
                    idx = cv_node_sum_f32(sum, tilted, po, k) < k->threshold * vnf ? c->node_left[n0 + idx] : c->node_right[n0 + idx];
                } while (idx > 0);
                stage_sum += c->alpha[c->tree_first_alpha[t] - idx];
            }
            if (stage_sum >= c->stage_threshold[ptr] - 0.0001f) {
                ptr = c->stage_child[ptr];
            } else {
                while (ptr != -1 && c->stage_next[ptr] == -1) ptr = c->stage_parent[ptr];
                if (ptr == -1) { *stage_sum_out = stage_sum; return 0; }
                ptr = c->stage_next[ptr];
            }
        }
        *stage_sum_out = stage_sum;
        return 1;
    }
    for (int i = 0; i < c->n_stages; ++i) {                                          /* :862-966 */
        stage_sum = 0.0;
        for (int t = c->stage_first_tree[i]; t < c->stage_first_tree[i] + c->stage_n_trees[i]; ++t) {
            const int n0 = c->tree_first_node[t];
            const float* alpha = c->alpha + c->tree_first_alpha[t];
            if (s->is_stump_based) {
                const cv_node* k = kn + n0;
                const double tt = k->threshold * vnf;
                double v;
                if (s->two_rects[i]) {                                               /* :872-888 */
                    const int32_t* img = k->tilted ? tilted : sum;
                    double rect0 = cv_calc_sum(img, po, &k->rect[0]);
                    rect0 *= k->rect[0].weight;
                    double rect1 = cv_calc_sum(img, po, &k->rect[1]);
                    rect1 *= k->rect[1].weight;
                    v = rect1 + rect0;
                } else {                                                             /* :901-913 */
                    v = cv_node_sum_f32(sum, tilted, po, k);
                }
                stage_sum += alpha[v >= tt];
            } else {                                                                 /* :952-961 */
                int idx = 0;
                do {
                    const cv_node* k = kn + n0 + idx;
                    idx = cv_node_sum_f32(sum, tilted, po, k) < k->threshold * vnf ? c->node_left[n0 + idx] : c->node_right[n0 + idx];
                } while (idx > 0);
                stage_sum += alpha[-idx];
            }
        }
        if (stage_sum < c->stage_threshold[i] - 0.0001f) { *stage_sum_out = stage_sum; return -i; }
    }
    *stage_sum_out = stage_sum;
    return 1;
}

/* Raw lists in the reference's order: level by level, y then x.  out / levels / weights hold `cap` entries; *n_total counts all
 * reports, *n_levels the evaluated levels.  max_w or max_h == 0: maxSize is the image. */
int roc_detect(const oc_cascade* c, const uint8_t* gray, int W, int H, int stride, int min_w, int min_h, int max_w, int max_h, double scaleFactor,
               oc_rect* out, int32_t* levels, double* weights, int cap, int* n_total, int* n_levels) {
    si_setup s;
    s.kn = (cv_node*)malloc(sizeof(cv_node) * (size_t)c->n_nodes);
    si_flags(c, &s);
    if (max_h == 0 || max_w == 0) { max_h = H; max_w = W; }                          /* :1230-1234 */
    uint8_t* small = (uint8_t*)malloc((size_t)W * H);
    int found = 0, n_lv = 0, scale_idx = 0;
    for (double factor = 1;; factor *= scaleFactor, ++scale_idx) {                   /* :1268-1288 */
        const int win_w = cv_round(c->win_w * factor), win_h = cv_round(c->win_h * factor);
        const int w = cv_round(W / factor), h = cv_round(H / factor);
        if (w - c->win_w + 1 <= 0 || h - c->win_h + 1 <= 0) break;
        if (win_w > max_w || win_h > max_h) break;
        if (win_w < min_w || win_h < min_h) continue;
        ++n_lv;
        si_resize_linear(gray, W, H, stride, small, w, h, w);
        const int sw = w + 1;
        int32_t* sum = (int32_t*)calloc((size_t)sw * (h + 1), sizeof(int32_t));
        double* sqsum = (double*)calloc((size_t)sw * (h + 1), sizeof(double));
        int32_t* tilted = NULL;
        oc_integral(small, w, h, w, sum, sqsum);
        if (s.has_tilted) {
            tilted = (int32_t*)calloc((size_t)sw * (h + 1), sizeof(int32_t));
            oc_integral_tilted(small, w, h, w, tilted);
        }
        si_set_images(c, w, &s);
        const int ystep = factor > 2 ? 1 : 2;                                        /* :1304 */
        for (int y = 0; y < h - c->win_h; y += ystep)                                /* :1079-1095 (the grid: :1015-1020) */
            for (int x = 0; x < w - c->win_w; x += ystep) {
                double gypWeight = 0.0;
                int result = roc_run(c, &s, sum, sqsum, tilted, sw, x, y, &gypWeight);
                if (result == 1) result = -1 * c->n_stages;
                if (c->n_stages + result < 4) {
                    if (found < cap) {
                        out[found].x = cv_round(x * factor);
                        out[found].y = cv_round(y * factor);
                        out[found].w = win_w;
                        out[found].h = win_h;
                        out[found].scale_idx = scale_idx;
                        levels[found] = -result;
                        weights[found] = gypWeight;
                    }
                    ++found;
                }
            }
        free(sum); free(sqsum); free(tilted);
    }
    free(small); free(s.kn);
    *n_total = found;
    *n_levels = n_lv;
    return found < cap ? found : cap;
}

/* AgroupRectangles(rectList, groupThreshold, eps, &rejectLevels, &levelWeights) (:145-243), in place; returns the new count */
int roc_group(oc_grect* rects, int32_t* levels, double* lweights, int n, int groupThreshold, double eps) {
    if (groupThreshold <= 0 || n == 0) {                                             /* :147-157: "weights" are the levels here */
        for (int i = 0; i < n; i++) levels[i] = 1;
        return n;
    }
    int* labels = (int*)malloc(sizeof(int) * (size_t)n);
    const int nclasses = oc_partition(rects, n, eps, labels);
    oc_grect* rrects = (oc_grect*)calloc((size_t)nclasses, sizeof(oc_grect));
    int* rweights = (int*)calloc((size_t)nclasses, sizeof(int));
    int* rejectLevels = (int*)calloc((size_t)nclasses, sizeof(int));
    double* rejectWeights = (double*)malloc(sizeof(double) * (size_t)nclasses);
    for (int i = 0; i < nclasses; i++) rejectWeights[i] = DBL_MIN;
    for (int i = 0; i < n; i++) {
        const int cls = labels[i];
        rrects[cls].x += rects[i].x; rrects[cls].y += rects[i].y;
        rrects[cls].w += rects[i].w; rrects[cls].h += rects[i].h;
        rweights[cls]++;
    }
    for (int i = 0; i < n; i++) {                                                    /* :176-189 (both vectors are non-empty: n != 0) */
        const int cls = labels[i];
        if (levels[i] > rejectLevels[cls]) {
            rejectLevels[cls] = levels[i];
            rejectWeights[cls] = lweights[i];
        } else if (levels[i] == rejectLevels[cls] && lweights[i] > rejectWeights[cls]) {
            rejectWeights[cls] = lweights[i];
        }
    }
    for (int i = 0; i < nclasses; i++) {
        const oc_grect r = rrects[i];
        const float s = 1.f / rweights[i];
        rrects[i].x = r.x * s > 2147483647 ? 2147483647 : (int)(r.x * s);
        rrects[i].y = r.y * s > 2147483647 ? 2147483647 : (int)(r.y * s);
        rrects[i].w = r.w * s > 2147483647 ? 2147483647 : (int)(r.w * s);
        rrects[i].h = r.h * s > 2147483647 ? 2147483647 : (int)(r.h * s);
    }
    int out = 0;
    for (int i = 0; i < nclasses; i++) {
        const oc_grect r1 = rrects[i];
        const int n1 = rejectLevels[i];                                              /* :210: the LEVEL */
        const double w1 = rejectWeights[i];
        int j;
        if (n1 <= groupThreshold) continue;
        for (j = 0; j < nclasses; j++) {
            const int n2 = rweights[j];                                              /* :217: the member COUNT */
            if (j == i || n2 <= groupThreshold) continue;
            const oc_grect r2 = rrects[j];
            const int dx = r2.w * eps > 2147483647 ? 2147483647 : (int)(r2.w * eps);
            const int dy = r2.h * eps > 2147483647 ? 2147483647 : (int)(r2.h * eps);
            if (r1.x >= r2.x - dx && r1.y >= r2.y - dy && r1.x + r1.w <= r2.x + r2.w + dx && r1.y + r1.h <= r2.y + r2.h + dy &&
                (n2 > (3 > n1 ? 3 : n1) || n1 < 3))
                break;
        }
        if (j == nclasses) { rects[out] = r1; levels[out] = n1; lweights[out] = w1; out++; }   /* (the inputs are no longer read) */
    }
    free(labels); free(rrects); free(rweights); free(rejectLevels); free(rejectWeights);
    return out;
}
