/* Test restatement of the reference's public per-window pair (its private copy of OpenCV 2.4.2 haar.cpp) on top of
 * tests/scale_image_oracle.c (the hidden-cascade flags) and oracle/vj_oracle.c (integrals, calc_sum, the int * float node sum):
 *   rw_set_scale   cvSetImagesForHaarClassifierCascade(cascade, sum, sqsum, tilted, scale) (tempcv.cpp:549-768) at an ARBITRARY double
 *                  scale: real_window_size = cvRound(orig * scale) (:608-609), equRect (:614-616), inv_window_area (:617-618), the
 *                  cvRound-ed rectangles of every node with rect 0's weight derived from the others (:632-768; CV_ADJUST_WEIGHTS = 0,
 *                  and the "align blocks" flags can never be set)
 *   rw_run         cvRunHaarClassifierCascade(cascade, pt, start_stage) (:974-984) -> cvRunHaarClassifierCascadeSum (:795-972): the
 *                  border rule (:817-820), the variance norm factor (:822-832), the stage tree (:834-861, which asserts start_stage
 *                  == 0 at :837), stump stages in both arithmetic modes (:862-950) and multi-node trees (:951-966) from start_stage
 *                  on; returns the function's int and leaves in *stage_sum what the function leaves in its reference parameter
 *                  (0.0 where it never writes it)
 * Built by tests/run_window_oracle.py with the flags of tests/scale_image_oracle.py.                                         */
#include "scale_image_oracle.c"

#include <limits.h>

#define RW_WIN_MAX (1 << 20)   /* a window no frame holds; rounding is clamped there so that no scale overflows an int */

typedef struct rw_ctx {
    const oc_cascade* c;
    int W, H, sw;
    int32_t* sum;
    double* sqsum;
    int32_t* tilted;
    si_setup s;            /* flags, equRect corners, weight_scale, node records */
    int real_w, real_h;
    int fits;              /* some position passes the border rule */
} rw_ctx;

static int rw_round_clamped(double v) { return v < (double)RW_WIN_MAX ? cv_round(v) : RW_WIN_MAX; }

rw_ctx* rw_create(const oc_cascade* c, const uint8_t* gray, int W, int H, int stride) {
    rw_ctx* k = (rw_ctx*)calloc(1, sizeof(rw_ctx));
    k->c = c;
    k->W = W;
    k->H = H;
    k->sw = W + 1;
    /* two rows of zeroed slack below the integrals: a feature may overshoot its window by a row (separate rounding) */
    k->sum = (int32_t*)calloc((size_t)k->sw * (H + 3), sizeof(int32_t));
    k->sqsum = (double*)calloc((size_t)k->sw * (H + 3), sizeof(double));
    oc_integral(gray, W, H, stride, k->sum, k->sqsum);
    k->s.kn = (cv_node*)malloc(sizeof(cv_node) * (size_t)c->n_nodes);
    si_flags(c, &k->s);
    if (k->s.has_tilted) {
        k->tilted = (int32_t*)calloc((size_t)k->sw * (H + 3), sizeof(int32_t));
        oc_integral_tilted(gray, W, H, stride, k->tilted);
    }
    return k;
}

void rw_free(rw_ctx* k) {
    if (!k) return;
    free(k->sum); free(k->sqsum); free(k->tilted); free(k->s.kn); free(k);
}

int rw_is_tree(const rw_ctx* k) { return k->s.is_tree; }
int rw_two_rects(const rw_ctx* k, int stage) { return k->s.is_stump_based && !k->s.is_tree && k->s.two_rects[stage]; }

void rw_set_scale(rw_ctx* k, double scale) {                                         /* :549-768 */
    const oc_cascade* c = k->c;
    si_setup* s = &k->s;
    const int sw = k->sw;
    k->real_w = rw_round_clamped(c->win_w * scale);                                  /* :608-609 */
    k->real_h = rw_round_clamped(c->win_h * scale);
    k->fits = k->real_w <= k->W && k->real_h <= k->H;
    if (!k->fits) return;                                                            /* every window: -1; nothing below is read */
    const int ex = cv_round(scale), ew = cv_round((c->win_w - 2) * scale), eh = cv_round((c->win_h - 2) * scale);   /* :614-616 */
    s->weight_scale = 1. / (ew * eh);                                                /* :617-618 */
    s->q0 = ex * sw + ex;
    s->q1 = ex * sw + ex + ew;
    s->q2 = (ex + eh) * sw + ex;
    s->q3 = (ex + eh) * sw + ex + ew;
    for (int n = 0; n < c->n_nodes; ++n) {                                           /* :632-768 */
        cv_node* kn = s->kn + n;
        const int32_t* r2 = c->node_rect + (n * 3 + 2) * 4;
        double sum0 = 0, area0 = 0;
        kn->nrect = (fabs((double)c->node_weight[n * 3 + 2]) < DBL_EPSILON || r2[2] == 0 || r2[3] == 0) ? 2 : 3;
        kn->tilted = c->node_tilted ? c->node_tilted[n] != 0 : 0;
        kn->threshold = c->node_threshold[n];
        const double correction_ratio = s->weight_scale * (!kn->tilted ? 1 : 0.5);   /* :731 */
        for (int j = 0; j < kn->nrect; ++j) {
            const int32_t* r = c->node_rect + (n * 3 + j) * 4;
            const int tx = cv_round(r[0] * scale), ty = cv_round(r[1] * scale);
            const int tw = cv_round(r[2] * scale), th = cv_round(r[3] * scale);
            if (!kn->tilted) {                                                       /* :735-741 */
                kn->rect[j].p0 = ty * sw + tx;
                kn->rect[j].p1 = ty * sw + tx + tw;
                kn->rect[j].p2 = (ty + th) * sw + tx;
                kn->rect[j].p3 = (ty + th) * sw + tx + tw;
            } else {                                                                 /* :743-750 */
                kn->rect[j].p2 = (ty + tw) * sw + tx + tw;
                kn->rect[j].p3 = (ty + tw + th) * sw + tx + tw - th;
                kn->rect[j].p0 = ty * sw + tx;
                kn->rect[j].p1 = (ty + th) * sw + tx - th;
            }
            kn->rect[j].weight = (float)(c->node_weight[n * 3 + j] * correction_ratio);
            if (j == 0) area0 = tw * th;
            else sum0 += kn->rect[j].weight * tw * th;                               /* :756 */
        }
        kn->rect[0].weight = (float)(-sum0 / area0);                                 /* :767 */
    }
}

/* INT_MIN: the reference's assert (a stage tree with start_stage != 0, or a negative start_stage) */
int rw_run(const rw_ctx* k, int x, int y, int start_stage, double* stage_sum_out) {
    const oc_cascade* c = k->c;
    const si_setup* s = &k->s;
    const cv_node* kn = s->kn;
    const int sw = k->sw;
    *stage_sum_out = 0.0;
    if (start_stage < 0 || (s->is_tree && start_stage != 0)) return INT_MIN;             /* :837 */
    if (x < 0 || y < 0 || (long long)x + k->real_w >= (long long)k->W + 1 || (long long)y + k->real_h >= (long long)k->H + 1)
        return -1;                                                                   /* :817-820 (sum.width = W + 1) */
    const int po = y * sw + x;
    const int32_t* sum = k->sum;
    const int32_t* tilted = k->tilted;
    const double mean = (double)(int)((uint32_t)sum[po + s->q0] - (uint32_t)sum[po + s->q1] - (uint32_t)sum[po + s->q2] + (uint32_t)sum[po + s->q3]) *
                        s->weight_scale;                                             /* :824-825 */
    double vnf = k->sqsum[po + s->q0] - k->sqsum[po + s->q1] - k->sqsum[po + s->q2] + k->sqsum[po + s->q3];
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
                do {                                                                 /* icvEvalHidHaarClassifier, :771-792 */
                    const cv_node* nd = kn + n0 + idx;
                    idx = cv_node_sum_f32(sum, tilted, po, nd) < nd->threshold * vnf ? c->node_left[n0 + idx] : c->node_right[n0 + idx];
                } while (idx > 0);
                stage_sum += c->alpha[c->tree_first_alpha[t] - idx];
            }
            *stage_sum_out = stage_sum;
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
    for (int i = start_stage; i < c->n_stages; ++i) {                                /* :864, :952 */
        stage_sum = 0.0;
        for (int t = c->stage_first_tree[i]; t < c->stage_first_tree[i] + c->stage_n_trees[i]; ++t) {
            const int n0 = c->tree_first_node[t];
            const float* alpha = c->alpha + c->tree_first_alpha[t];
            if (s->is_stump_based) {
                const cv_node* nd = kn + n0;
                const double tt = nd->threshold * vnf;
                double v;
                if (s->two_rects[i]) {                                               /* :872-888 */
                    const int32_t* img = nd->tilted ? tilted : sum;
                    double rect0 = cv_calc_sum(img, po, &nd->rect[0]);
                    rect0 *= nd->rect[0].weight;
                    double rect1 = cv_calc_sum(img, po, &nd->rect[1]);
                    rect1 *= nd->rect[1].weight;
                    v = rect1 + rect0;
                } else {                                                             /* :901-913 */
                    v = cv_node_sum_f32(sum, tilted, po, nd);
                }
                stage_sum += alpha[v >= tt];
            } else {                                                                 /* :952-961 */
                int idx = 0;
                do {
                    const cv_node* nd = kn + n0 + idx;
                    idx = cv_node_sum_f32(sum, tilted, po, nd) < nd->threshold * vnf ? c->node_left[n0 + idx] : c->node_right[n0 + idx];
                } while (idx > 0);
                stage_sum += alpha[-idx];
            }
        }
        *stage_sum_out = stage_sum;
        if (stage_sum < c->stage_threshold[i] - 0.0001f) return -i;                  /* :947-949, :963-965 */
    }
    return 1;
}

/* rw_run on n points (xy: n x 2 ints) at the scale last set */
void rw_run_list(const rw_ctx* k, const int32_t* xy, int n, int start_stage, int32_t* results, double* sums) {
    for (int i = 0; i < n; ++i) results[i] = rw_run(k, xy[2 * i], xy[2 * i + 1], start_stage, sums + i);
}
