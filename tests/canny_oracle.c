/* Test restatement of CV_HAAR_DO_CANNY_PRUNING (cvHaarDetectObjects' flags bit 0, tempcv.hpp:127) on top of the CPU oracle:
 *   cn_canny                 cvCanny(gray, edges, 0, 50, 3) as DESIGN.md §4.7 states it (OpenCV 2.4.2 imgproc: third-party,
 *                            parity unpinned) — Sobel with replicated borders, |dx| + |dy|, non-maximum suppression with
 *                            TG22 = 13573, candidates m > 0, strong m > 50, hysteresis as a flood fill from the strong pixels
 *                            (a different algorithm from the device's union-find: the edge SET is what is specified)
 *   cn_detect_opencvlike     the oracle's detect_opencvlike_impl walk with the pruning test of tempcv.cpp:1147-1158 in front
 *                            of the border rule; prune = 0 is that walk unchanged (the anchor test compares the two)
 * Built by tests/canny_oracle.py with oracle/Makefile's flags.  oracle/ itself is not modified.                          */
#include "../oracle/vj_oracle.c"

static inline int cn_g(const uint8_t* gray, int W, int H, int stride, int x, int y) {
    x = x < 0 ? 0 : x >= W ? W - 1 : x;
    y = y < 0 ? 0 : y >= H ? H - 1 : y;
    return gray[(size_t)y * stride + x];
}

/* edges: W x H bytes, rows of edges_stride, 255 / 0 */
void cn_canny(const uint8_t* gray, int W, int H, int stride, uint8_t* edges, int edges_stride) {
    const int mw = W + 2;
    int* mag = (int*)calloc((size_t)mw * (H + 2), sizeof(int));     /* m with a ring of zeros: m = 0 at x = -1, W and y = -1, H */
    int* dxs = (int*)malloc(sizeof(int) * (size_t)W * H);
    int* dys = (int*)malloc(sizeof(int) * (size_t)W * H);
    uint8_t* cls = (uint8_t*)calloc((size_t)W * H, 1);
    int* stack = (int*)malloc(sizeof(int) * (size_t)W * H);
#define M(x, y) mag[(size_t)((y) + 1) * mw + (x) + 1]
#define G(x, y) cn_g(gray, W, H, stride, (x), (y))
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int dx = (G(x + 1, y - 1) - G(x - 1, y - 1)) + 2 * (G(x + 1, y) - G(x - 1, y)) + (G(x + 1, y + 1) - G(x - 1, y + 1));
            const int dy = (G(x - 1, y + 1) - G(x - 1, y - 1)) + 2 * (G(x, y + 1) - G(x, y - 1)) + (G(x + 1, y + 1) - G(x + 1, y - 1));
            dxs[(size_t)y * W + x] = dx;
            dys[(size_t)y * W + x] = dy;
            M(x, y) = abs(dx) + abs(dy);
        }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int m = M(x, y);
            if (!(m > 0)) continue;
            const int dx = dxs[(size_t)y * W + x], dy = dys[(size_t)y * W + x];
            const int ax = abs(dx), ay = abs(dy) << 15;
            const int tg22x = ax * 13573, tg67x = tg22x + (ax << 16);
            int cand;
            if (ay < tg22x) cand = m > M(x - 1, y) && m >= M(x + 1, y);
            else if (ay > tg67x) cand = m > M(x, y - 1) && m >= M(x, y + 1);
            else {
                const int s = (dx ^ dy) < 0 ? -1 : 1;
                cand = m > M(x - s, y - 1) && m > M(x + s, y + 1);
            }
            if (cand) cls[(size_t)y * W + x] = m > 50 ? 2 : 1;
        }
#undef M
#undef G
    for (int y = 0; y < H; ++y) memset(edges + (size_t)y * edges_stride, 0, (size_t)W);
    int top = 0;
    for (int i = 0; i < W * H; ++i)
        if (cls[i] == 2) {
            edges[(size_t)(i / W) * edges_stride + i % W] = 255;
            stack[top++] = i;
        }
    while (top > 0) {
        const int i = stack[--top], x = i % W, y = i / W;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int nx = x + dx, ny = y + dy;
                if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
                uint8_t* e = edges + (size_t)ny * edges_stride + nx;
                if (cls[(size_t)ny * W + nx] && !*e) {
                    *e = 255;
                    stack[top++] = ny * W + nx;
                }
            }
    }
    free(mag); free(dxs); free(dys); free(cls); free(stack);
}

/* detect_opencvlike_impl (oracle/vj_oracle.c) with `prune` (1; 2 = the test without its sq < 20 clause, for tests): returns -1 if a pruning rectangle would read past the frame's
 * (H + 3)-row integral allocation (the library refuses such a call with VJ_ERR_LIMIT). */
int cn_detect_opencvlike(const oc_cascade* c, const uint8_t* gray, int W, int H, int stride, int min_w, int min_h,
                         double scaleFactor, int prune, oc_rect* out, int cap, int* n_total, oc_stats* st) {
    const int sw = W + 1;
    const size_t elems = (size_t)sw * (H + 3);
    int32_t* sum = (int32_t*)calloc(elems, sizeof(int32_t));
    double* sqsum = (double*)calloc(elems, sizeof(double));
    int32_t* esum = NULL;
    int32_t* tilted = NULL;
    cv_node* kn = (cv_node*)malloc(sizeof(cv_node) * (size_t)c->n_nodes);
    int rc = 0;
    memset(st, 0, sizeof(*st));
    g_all_f64 = 0;
    oc_integral(gray, W, H, stride, sum, sqsum);
    if (prune) {
        uint8_t* edges = (uint8_t*)malloc((size_t)W * H);
        double* scratch = (double*)calloc(elems, sizeof(double));
        esum = (int32_t*)calloc(elems, sizeof(int32_t));
        cn_canny(gray, W, H, stride, edges, W);
        oc_integral(edges, W, H, W, esum, scratch);
        free(edges);
        free(scratch);
    }
    int is_stump_based = 1, is_tree = 0, has_tilted = 0;
    int two_rects[64];
    for (int t = 0; t < c->n_trees; ++t) is_stump_based &= c->tree_n_nodes[t] == 1;
    for (int i = 0; i < c->n_stages && i < 64; ++i) {
        is_tree |= c->stage_next[i] != -1;
        two_rects[i] = 1;
        const int t0 = c->stage_first_tree[i], t1 = t0 + c->stage_n_trees[i];
        for (int t = t0; t < t1; ++t)
            for (int l = 0; l < c->tree_n_nodes[t]; ++l) {
                const int n = c->tree_first_node[t] + l;
                const int32_t* r2 = c->node_rect + (n * 3 + 2) * 4;
                if (!(fabs((double)c->node_weight[n * 3 + 2]) < 2.220446049250313e-16 || r2[2] == 0 || r2[3] == 0))
                    two_rects[i] = 0;
                if (c->node_tilted && c->node_tilted[n]) has_tilted = 1;
            }
    }
    if (has_tilted) {
        tilted = (int32_t*)calloc(elems, sizeof(int32_t));
        oc_integral_tilted(gray, W, H, stride, tilted);
    }
    int found = 0, n_factors = 0, scale_index = 0;
    double factor;
    for (n_factors = 0, factor = 1; factor * c->win_w < W - 10 && factor * c->win_h < H - 10;
         n_factors++, factor *= scaleFactor) {}
    factor = 1;
    for (; n_factors-- > 0 && rc == 0; factor *= scaleFactor, scale_index++) {
        const double ystep = 2. > factor ? 2. : factor;
        const int win_w = cv_round(c->win_w * factor), win_h = cv_round(c->win_h * factor);
        const int endX = cv_round((W - win_w) / ystep), endY = cv_round((H - win_h) / ystep);
        if (win_w < min_w || win_h < min_h) continue;
        const int ex = cv_round(factor), ew = cv_round((c->win_w - 2) * factor), eh = cv_round((c->win_h - 2) * factor);
        const double weight_scale = 1. / (ew * eh);
        const int q0 = ex * sw + ex, q1 = ex * sw + ex + ew, q2 = (ex + eh) * sw + ex, q3 = (ex + eh) * sw + ex + ew;
        /* tempcv.cpp:1147-1158: the pruning rectangle of the scaled window */
        const int px = cv_round(win_w * 0.15), py = cv_round(win_h * 0.15), pw = cv_round(win_w * 0.7), ph = cv_round(win_h * 0.7);
        const int e0 = py * sw + px, e1 = e0 + pw, e2 = (py + ph) * sw + px, e3 = e2 + pw;
        for (int n = 0; n < c->n_nodes; ++n) {
            double sum0 = 0, area0 = 0;
            const int32_t* r2 = c->node_rect + (n * 3 + 2) * 4;
            const int nr = (fabs((double)c->node_weight[n * 3 + 2]) < 2.220446049250313e-16 || r2[2] == 0 || r2[3] == 0) ? 2 : 3;
            kn[n].nrect = nr;
            kn[n].tilted = c->node_tilted ? c->node_tilted[n] != 0 : 0;
            kn[n].threshold = c->node_threshold[n];
            const double correction_ratio = weight_scale * (!kn[n].tilted ? 1 : 0.5);
            for (int k = 0; k < nr; ++k) {
                const int32_t* r = c->node_rect + (n * 3 + k) * 4;
                const int tx = cv_round(r[0] * factor), ty = cv_round(r[1] * factor);
                const int tw = cv_round(r[2] * factor), th = cv_round(r[3] * factor);
                if (!kn[n].tilted) {
                    kn[n].rect[k].p0 = ty * sw + tx;
                    kn[n].rect[k].p1 = ty * sw + tx + tw;
                    kn[n].rect[k].p2 = (ty + th) * sw + tx;
                    kn[n].rect[k].p3 = (ty + th) * sw + tx + tw;
                } else {
                    kn[n].rect[k].p2 = (ty + tw) * sw + tx + tw;
                    kn[n].rect[k].p3 = (ty + tw + th) * sw + tx + tw - th;
                    kn[n].rect[k].p0 = ty * sw + tx;
                    kn[n].rect[k].p1 = (ty + th) * sw + tx - th;
                }
                kn[n].rect[k].weight = (float)(c->node_weight[n * 3 + k] * correction_ratio);
                if (k == 0) area0 = tw * th;
                else sum0 += kn[n].rect[k].weight * tw * th;
            }
            kn[n].rect[0].weight = (float)(-sum0 / area0);
        }
        for (int iy = 0; iy < endY && rc == 0; iy++) {
            const int y = cv_round(iy * ystep);
            int ixstep = 1;
            for (int ix = 0; ix < endX; ix += ixstep) {
                const int x = cv_round(ix * ystep);
                int result;
                st->windows++;
                if (prune) {
                    const int po = y * sw + x;
                    if ((size_t)po + (size_t)e3 >= elems) { rc = -1; break; }
                    const int s = (int)((uint32_t)esum[po + e0] - (uint32_t)esum[po + e1] - (uint32_t)esum[po + e2] + (uint32_t)esum[po + e3]);
                    const int sq = (int)((uint32_t)sum[po + e0] - (uint32_t)sum[po + e1] - (uint32_t)sum[po + e2] + (uint32_t)sum[po + e3]);
                    if (s < 100 || (prune != 2 && sq < 20)) {   /* prune = 2: without the sq clause (a test knob, NOT OpenCV) */
                        ixstep = 2;
                        continue;
                    }
                }
                if (x < 0 || y < 0 || x + win_w >= sw || y + win_h >= H + 1) {
                    result = -1;
                } else {
                    const int po = y * sw + x;
                    double mean = (double)(int)((uint32_t)sum[po + q0] - (uint32_t)sum[po + q1] - (uint32_t)sum[po + q2] +
                                                (uint32_t)sum[po + q3]) * weight_scale;
                    double vnf = sqsum[po + q0] - sqsum[po + q1] - sqsum[po + q2] + sqsum[po + q3];
                    vnf = vnf * weight_scale - mean * mean;
                    vnf = vnf >= 0. ? sqrt(vnf) : 1.;
                    if (is_tree) {
                        int ptr = 0;
                        result = 1;
                        while (ptr != -1) {
                            double stage_sum = 0.0;
                            const int t0 = c->stage_first_tree[ptr], t1 = t0 + c->stage_n_trees[ptr];
                            st->stage_entered[ptr]++;
                            for (int t = t0; t < t1; ++t) {
                                const int n0 = c->tree_first_node[t];
                                const float* alpha = c->alpha + c->tree_first_alpha[t];
                                int idx = 0;
                                do {
                                    const cv_node* k = kn + n0 + idx;
                                    const double tt = k->threshold * vnf;
                                    const double s = cv_node_sum_f32(sum, tilted, po, k);
                                    st->stump_evals++;
                                    idx = s < tt ? c->node_left[n0 + idx] : c->node_right[n0 + idx];
                                } while (idx > 0);
                                stage_sum += alpha[-idx];
                            }
                            if (stage_sum >= c->stage_threshold[ptr] - 0.0001f) {
                                ptr = c->stage_child[ptr];
                            } else {
                                while (ptr != -1 && c->stage_next[ptr] == -1) ptr = c->stage_parent[ptr];
                                if (ptr == -1) { result = 0; break; }
                                ptr = c->stage_next[ptr];
                            }
                        }
                    } else {
                        result = 1;
                        for (int i = 0; i < c->n_stages; ++i) {
                            double stage_sum = 0.0;
                            const int t0 = c->stage_first_tree[i], t1 = t0 + c->stage_n_trees[i];
                            st->stage_entered[i]++;
                            for (int t = t0; t < t1; ++t) {
                                const int n0 = c->tree_first_node[t];
                                const float* alpha = c->alpha + c->tree_first_alpha[t];
                                if (is_stump_based) {
                                    const cv_node* k = kn + n0;
                                    const double tt = k->threshold * vnf;
                                    double s;
                                    st->stump_evals++;
                                    if (two_rects[i]) {
                                        const int32_t* img = k->tilted ? tilted : sum;
                                        double rect0 = cv_calc_sum(img, po, &k->rect[0]);
                                        rect0 *= k->rect[0].weight;
                                        double rect1 = cv_calc_sum(img, po, &k->rect[1]);
                                        rect1 *= k->rect[1].weight;
                                        s = rect1 + rect0;
                                    } else {
                                        s = cv_node_sum_f32(sum, tilted, po, k);
                                    }
                                    stage_sum += alpha[s >= tt];
                                } else {
                                    int idx = 0;
                                    do {
                                        const cv_node* k = kn + n0 + idx;
                                        const double tt = k->threshold * vnf;
                                        const double s = cv_node_sum_f32(sum, tilted, po, k);
                                        st->stump_evals++;
                                        idx = s < tt ? c->node_left[n0 + idx] : c->node_right[n0 + idx];
                                    } while (idx > 0);
                                    stage_sum += alpha[-idx];
                                }
                            }
                            if (stage_sum < c->stage_threshold[i] - 0.0001f) { result = -i; break; }
                        }
                    }
                }
                if (result > 0) {
                    if (found < cap) { out[found].x = x; out[found].y = y; out[found].w = win_w; out[found].h = win_h; out[found].scale_idx = scale_index; }
                    found++;
                }
                ixstep = result != 0 ? 1 : 2;
            }
        }
    }
    free(kn); free(sum); free(sqsum); free(tilted); free(esum);
    *n_total = found;
    if (rc) return rc;
    return found < cap ? found : cap;
}
