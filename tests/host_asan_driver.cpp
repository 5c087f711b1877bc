// Sanitizer driver of the library's host-side sources (cascade parser / loader, scale and feature-table planning, the plan
// builders of the clod and the OpenCV profile, sharding helpers, rectangle grouping): built by tests/test_sanitizers.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/host_asan_driver.cpp csrc/vj_cascade.cpp csrc/vj_plan.cpp csrc/vj_clod_plan.cpp csrc/vj_group.cpp
//       csrc/vj_cv_plan.cpp csrc/vj_cv_roi_host.cpp csrc/vj_cv_roi_levels_host.cpp
// (no HIP involved — GPU AddressSanitizer is not available on the pool).  Malformed and truncated inputs must come back
// as error codes; every memory error or undefined behaviour aborts the process.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../include/vj.h"
#include "../clfacedetection_amd/csrc/vj_cv_plan.hpp"

static uint32_t rng_state = 1;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static std::string slurp(const std::string& path) {
    std::string s;
    if (FILE* f = fopen(path.c_str(), "rb")) {
        char buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
        fclose(f);
    }
    return s;
}
static void spit(const std::string& path, const std::string& s) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    fwrite(s.data(), 1, s.size(), f);
    fclose(f);
}

// The whole clod plan (vj_clod_plan.cpp) of a frame size through the host-only query, with VJ_FLAG_TILTED_AS_UPRIGHT so that
// a tilted feature does not end the query before any table is built (main asks once without it).  The chain balance, the batch
// size and the query flag rotate from call to call with periods 4, 8 and 3: every 24 calls meet each combination of the three
// once.  Error codes are fine, the sanitizers watch the index arithmetic; main prints how many queries gave a plan.
static int plans_ok = 0, plans_refused = 0;
static void plan(const vj_cascade* c, int W, int H, const vj_params* params) {
    static unsigned turn = 0;
    vj_params upright = *params;
    upright.flags |= VJ_FLAG_TILTED_AS_UPRIGHT;
    const vj_params* p = &upright;
    const float splits[] = {-1.0f, 0.0f, 0.5f, 3.3f};
    const uint32_t flags[] = {0u, VJ_PLAN_TILES_NO_GROUPS, VJ_PLAN_TILES_FORMER_SHAPES};
    std::vector<vj_tile_info> tiles(256);
    std::vector<uint64_t> gather(256);
    vj_tile_plan_info info;
    vj_tile_cut_info cut;
    int n = 0;
    const int rc = vj_plan_tiles_split(c, W, H, p, (turn / 4u) % 2u ? 64 : 1, flags[turn % 3u], splits[turn % 4u], &info, &cut, tiles.data(), gather.data(), 256, &n);
    ++(rc == VJ_OK ? plans_ok : plans_refused);
    ++turn;
}

// The whole plan of the OpenCV profile (plan_cv, vj_cv_plan.cpp) of a frame size under the default settings, for a call of at
// most four frames and for a larger one.  The mode rotates from call to call: plain, canny pruning, scale-image, find-biggest,
// scale-image with a ROC maxSize of half the frame.  Error codes are fine; what a plan promises its kernels is checked below,
// and a broken promise ends the run.
static int cv_plans_ok[5] = {}, cv_plans_refused = 0;
#define CV_CHECK(cond)                                                                                          \
    do {                                                                                                        \
        if (!(cond)) {                                                                                          \
            fprintf(stderr, "plan_cv, %d x %d mode %d small_batch %d: %s (line %d)\n", W, H, mode, (int)small_batch, #cond, __LINE__); \
            exit(1);                                                                                            \
        }                                                                                                       \
    } while (0)
static void check_cv_plan(const vj_cascade* c, int W, int H, int mode, bool small_batch, const vj::CvPlanHost& pl, const vj::CvPlanTables& tab) {
    using namespace vj;
    const uint32_t images = pl.has_tilted ? 2u : 1u;
    const size_t n_nodes = c->nodes.size();
    // LDS cap: what two (class 0) or one (class 1) tile workgroups may take next to the row kernel's
    for (int cls = 0; cls < 2; ++cls)
        CV_CHECK((int64_t)pl.class_lds[cls] <= (160 * 1024 - (int64_t)pl.row_blocks * 20 * 1024 - 1024) / (cls == 0 ? 2 : 1));
    CV_CHECK(pl.class_first[0] == 0u && pl.class_first[0] <= pl.class_first[1] && pl.class_first[1] <= pl.class_first[2] &&
             pl.class_first[2] == tab.tiles.size());
    std::vector<int> cls_of(pl.scales.size(), -1);
    std::vector<std::set<uint32_t>> origins(pl.scales.size());
    for (size_t i = 0; i < tab.tiles.size(); ++i) {
        const UnitDev& u = tab.tiles[i];
        CV_CHECK(u.scale < pl.scales.size());
        const CvScaleDev& sd = pl.scales[u.scale];
        const int cls = i < pl.class_first[1] ? 0 : 1;
        CV_CHECK(cls_of[u.scale] == -1 || cls_of[u.scale] == cls);
        cls_of[u.scale] = cls;
        // tile coverage, part 1: distinct origins on the tile grid, inside the window grid
        CV_CHECK(sd.tile_th != 0u && sd.tile_tw != 0u);
        const uint32_t ix0 = u.first & 0xffffu, iy0 = u.first >> 16;
        CV_CHECK(ix0 < sd.end_x && iy0 < sd.end_y && ix0 % sd.tile_tw == 0u && iy0 % sd.tile_th == 0u);
        CV_CHECK(origins[u.scale].insert(u.first).second);
    }
    uint32_t n_tile_scales = 0;
    for (size_t k = 0; k < pl.scales.size(); ++k) {
        const CvScaleDev& sd = pl.scales[k];
        if (sd.tile_th == 0u) {
            CV_CHECK(origins[k].empty());
            continue;
        }
        ++n_tile_scales;
        // tile coverage, part 2: as many of them as the grid has tiles — every window in exactly one
        CV_CHECK(origins[k].size() == (size_t)((sd.end_x + sd.tile_tw - 1u) / sd.tile_tw) * ((sd.end_y + sd.tile_th - 1u) / sd.tile_th));
        // LDS budget of the scale's class
        const uint64_t tile_elems = (uint64_t)sd.tile_pitch * sd.tile_rows * images;
        CV_CHECK(cls_of[k] >= 0 && (uint64_t)CVT_LDS_HEADER + tile_elems * 4u <= pl.class_lds[cls_of[k]]);
        // tile-pitch reach: every corner of every record, from the origin of the tile's last window, lies inside the staged images
        CV_CHECK((uint64_t)sd.tile_table_first + n_nodes <= tab.table.size());
        const uint64_t last_origin = ((uint64_t)std::ceil((double)(sd.tile_th - 1u) * sd.ystep) + 1u) * sd.tile_pitch + (uint64_t)std::ceil((double)(sd.tile_tw - 1u) * sd.ystep) + 1u;
        for (size_t n = 0; n < n_nodes; ++n) {
            const CvNodeRec& r = tab.table[sd.tile_table_first + n];
            for (int q = 0; q < 3; ++q)
                if (q < 2 || r.w[2] != 0.0f) CV_CHECK(last_origin + ((uint64_t)r.lt[q] + r.da[q] + r.db[q]) / 4u < tile_elems);
        }
    }
    CV_CHECK(n_tile_scales == pl.n_tile_scales);
    // row lists: rows_rest is rows without the tile scales' rows, in the same order
    size_t rest = 0;
    for (const UnitDev& r : tab.rows) {
        CV_CHECK(r.scale < pl.scales.size() && r.first < pl.scales[r.scale].end_y);
        if (pl.scales[r.scale].tile_th != 0u) continue;
        CV_CHECK(rest < tab.rows_rest.size() && memcmp(&tab.rows_rest[rest], &r, sizeof(r)) == 0);
        ++rest;
    }
    CV_CHECK(rest == tab.rows_rest.size() && pl.n_rows == tab.rows.size() && pl.n_rows_rest == tab.rows_rest.size());
    // bitmap segments: they tile [0, bits_frame_words) without gap or overlap
    uint32_t word = 0;
    for (const UnitDev& seg : tab.bit_segs) {
        CV_CHECK(seg.first == word && seg.count != 0u);
        word += seg.count;
    }
    CV_CHECK(word == pl.bits_frame_words && pl.n_bit_segs == tab.bit_segs.size());
    // canvas: the levels' rectangles lie inside it and do not overlap
    if (pl.scale_image) {
        CV_CHECK(tab.pyr_levels.size() == pl.scales.size() && pl.n_pyr_levels == pl.scales.size());
        for (size_t a = 0; a < tab.pyr_levels.size(); ++a) {
            const PyrLevelDev& la = tab.pyr_levels[a];
            CV_CHECK(la.w != 0u && la.h != 0u && la.ox + la.w <= pl.canvas_w && la.oy + la.h <= pl.canvas_h);
            CV_CHECK((uint64_t)la.ytab + la.h <= tab.pyr_taps.size());
            for (size_t b = 0; b < a; ++b) {
                const PyrLevelDev& lb = tab.pyr_levels[b];
                CV_CHECK(la.ox + la.w <= lb.ox || lb.ox + lb.w <= la.ox || la.oy + la.h <= lb.oy || lb.oy + lb.h <= la.oy);
            }
        }
    }
    // chains: the bounds are increasing and end at n_order
    CV_CHECK(pl.chains.n <= 4u);
    for (uint32_t k = 0; k < pl.chains.n; ++k) {
        CV_CHECK(pl.chains.begin[k] < pl.chains.end[k]);
        CV_CHECK(pl.chains.begin[k] == (k ? pl.chains.end[k - 1u] : pl.tree_prefix));
    }
    if (pl.chains.n) CV_CHECK(pl.chains.end[pl.chains.n - 1u] == pl.n_order);
}
static void cv_plan(const vj_cascade* c, int W, int H) {
    static unsigned turn = 0;
    const uint32_t flags[] = {0u, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_SCALE_IMAGE, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_SCALE_IMAGE};
    for (int sb = 0; sb < 2; ++sb, ++turn) {
        const int mode = (int)(turn % 5u);
        vj_cv_params p;
        memset(&p, 0, sizeof(p));
        p.scale_factor = 1.1;
        p.flags = flags[mode];
        const vj::CvMaxSize half{W / 2, H / 2};
        const vj::Tunables t;
        vj::CvPlanHost pl;
        vj::CvPlanTables tab;
        if (vj::plan_cv(t, c, W, H, p, sb != 0, mode == 4 ? &half : nullptr, &pl, &tab) != VJ_OK) {
            ++cv_plans_refused;
            continue;
        }
        ++cv_plans_ok[mode];
        check_cv_plan(c, W, H, mode, sb != 0, pl, tab);
    }
}

// everything the host does with a cascade once it is loaded
static void exercise(const vj_cascade* c) {
    vj_cascade_info info;
    if (vj_cascade_get_info(c, &info) != VJ_OK) return;
    vj_params p;
    vj_params_default(&p);
    for (int k = 0; k < 3; ++k) {
        const int W = 64 + (int)(rnd() % 700), H = 48 + (int)(rnd() % 500);
        int n = 0;
        std::vector<vj_scale_info> sc(256);
        if (vj_plan_scales(c, W, H, &p, sc.data(), 256, &n) != VJ_OK) continue;
        uint64_t wins = 0;
        (void)vj_count_windows(c, W, H, &p, &wins);
        uint64_t mask[2];
        for (int r = 0; r < 3; ++r) (void)vj_shard_scales(c, W, H, &p, 3, r, mask);
        std::vector<uint32_t> off((size_t)info.n_nodes * 12);
        std::vector<float> wts((size_t)info.n_nodes * 3);
        for (int i = 0; i < n && i < 256; i += 7)
            if (sc[(size_t)i].accepted) (void)vj_plan_feature_table(c, W, &sc[(size_t)i], off.data(), wts.data());
        plan(c, W, H, &p);
    }
    cv_plan(c, 1920, 1080);
    cv_plan(c, 100, 80);
}

static const char* kXml =
    "<?xml version=\"1.0\"?>\n<!-- a two-stage cascade -->\n<opencv_storage>\n<tiny type_id=\"opencv-haar-classifier\">\n"
    "  <size>20 20</size>\n  <stages>\n    <_>\n      <trees>\n        <_>\n          <_>\n            <feature>\n              <rects>\n"
    "                <_>3 7 14 4 -1.</_>\n                <_>3 9 14 2 2.</_></rects>\n              <tilted>0</tilted></feature>\n"
    "            <threshold>4.0141958743333817e-003</threshold>\n            <left_val>0.0337941907346249</left_val>\n"
    "            <right_val>0.8378106951713562</right_val></_></_>\n        <_>\n          <_>\n            <feature>\n              <rects>\n"
    "                <_>1 2 18 4 -1.</_>\n                <_>7 2 6 4 3.</_></rects>\n              <tilted>0</tilted></feature>\n"
    "            <threshold>0.0151513395830989</threshold>\n            <left_node>1</left_node>\n            <right_val>0.7488812208175659</right_val></_>\n"
    "          <_>\n            <feature>\n              <rects>\n                <_>9 2 9 9 -1.</_>\n                <_>9 5 9 3 3.</_></rects>\n"
    "              <tilted>1</tilted></feature>\n            <threshold>4.2109931819140911e-003</threshold>\n            <left_val>0.0900493934750557</left_val>\n"
    "            <right_val>0.6374819874763489</right_val></_></_></trees>\n      <stage_threshold>0.8226894140243530</stage_threshold>\n"
    "      <parent>-1</parent>\n      <next>-1</next></_>\n    <_>\n      <trees>\n        <_>\n          <_>\n            <feature>\n              <rects>\n"
    "                <_>5 6 10 6 -1.</_>\n                <_>5 8 10 2 3.</_></rects>\n              <tilted>0</tilted></feature>\n"
    "            <threshold>1.6227109590545297e-003</threshold>\n            <left_val>0.0693085864186287</left_val>\n"
    "            <right_val>0.7110946178436279</right_val></_></_></trees>\n      <stage_threshold>0.5</stage_threshold>\n"
    "      <parent>0</parent>\n      <next>-1</next></_></stages></tiny>\n</opencv_storage>\n";

int main(int argc, char** argv) {
    const std::string data = argc > 1 ? argv[1] : "clfacedetection_amd/data";
    const std::string tmp = argc > 2 ? argv[2] : "/tmp";
    const char* names[] = {"eye", "frontalface_alt", "frontalface_alt2", "frontalface_alt_tree", "frontalface_default", "fullbody",
                           "eye_tree_eyeglasses"};
    int loaded = 0, refused = 0;
    // 1. the shipped files load, survive a save / load round trip and the planning code
    for (const char* n : names) {
        const std::string path = data + "/haarcascade_" + n + ".vjc";
        vj_cascade* c = nullptr;
        if (vj_cascade_load(path.c_str(), &c) != VJ_OK) { fprintf(stderr, "cannot load %s: %s\n", path.c_str(), vj_last_error()); return 1; }
        exercise(c);
        vj_params tp;
        vj_params_default(&tp);
        plan(c, 1920, 1080, &tp);
        plan(c, 100, 80, &tp);
        const std::string rt = tmp + "/asan_rt.vjc";
        if (vj_cascade_save(c, rt.c_str()) != VJ_OK || slurp(rt) != slurp(path)) { fprintf(stderr, "round trip of %s differs\n", n); return 1; }
        // the in-memory constructor takes the same arrays
        vj_cascade_info info;
        vj_cascade_get_info(c, &info);
        vj_cascade* c2 = nullptr;
        if (vj_cascade_from_arrays(info.win_w, info.win_h, vj_cascade_stages(c), info.n_stages, vj_cascade_trees(c), info.n_trees,
                                   vj_cascade_nodes(c), info.n_nodes, vj_cascade_alpha(c), info.n_alpha, &c2) != VJ_OK) return 1;
        vj_cascade_free(c2);
        vj_cascade_free(c);
        ++loaded;
    }
    // ... and every shipped cascade gives a plan of the OpenCV profile in each of its modes
    const char* shipped[] = {"eye", "eye_tree_eyeglasses", "frontalface_alt", "frontalface_alt2", "frontalface_alt_tree", "frontalface_default",
                             "fullbody", "lefteye_2splits", "lowerbody", "mcs_eyepair_big", "mcs_eyepair_small", "mcs_lefteye", "mcs_mouth",
                             "mcs_nose", "mcs_righteye", "mcs_upperbody", "profileface", "righteye_2splits", "upperbody"};
    int before[5];
    memcpy(before, cv_plans_ok, sizeof(before));
    for (const char* n : shipped) {
        const std::string path = data + "/haarcascade_" + n + ".vjc";
        vj_cascade* c = nullptr;
        if (vj_cascade_load(path.c_str(), &c) != VJ_OK) { fprintf(stderr, "cannot load %s: %s\n", path.c_str(), vj_last_error()); return 1; }
        cv_plan(c, 1920, 1080);
        cv_plan(c, 100, 80);
        vj_cascade_free(c);
    }
    for (int mode = 0; mode < 5; ++mode)
        if (cv_plans_ok[mode] == before[mode]) { fprintf(stderr, "no shipped cascade gave a plan of the OpenCV profile in mode %d\n", mode); return 1; }
    // 2. truncated and corrupted .vjc files: an error code or a usable cascade, never a crash
    const std::string good = slurp(data + "/haarcascade_eye.vjc");
    const std::string bad = tmp + "/asan_bad.vjc";
    for (size_t len = 0; len < good.size(); len += (len < 400 ? 1 : 4099)) {
        spit(bad, good.substr(0, len));
        vj_cascade* c = nullptr;
        if (vj_cascade_load(bad.c_str(), &c) == VJ_OK) { fprintf(stderr, "a truncated file (%zu bytes) loaded\n", len); return 1; }
        ++refused;
    }
    for (int trial = 0; trial < 400; ++trial) {
        std::string m = good;
        const int flips = 1 + (int)(rnd() % 6);
        for (int k = 0; k < flips; ++k) {
            // mostly the header and the link structure (stage / tree / node records), where indices live
            const size_t pos = (rnd() % 4 == 0) ? rnd() % m.size() : rnd() % std::min<size_t>(m.size(), 60000);
            m[pos] = (char)(rnd() >> 11);
        }
        spit(bad, m);
        vj_cascade* c = nullptr;
        if (vj_cascade_load(bad.c_str(), &c) == VJ_OK) {
            exercise(c);
            vj_cascade_free(c);
            ++loaded;
        } else {
            ++refused;
        }
    }
    // 3. XML: the embedded cascade parses; every prefix and a few hundred mutations of it do not crash the parser
    const std::string xml = kXml, xpath = tmp + "/asan.xml";
    spit(xpath, xml);
    {
        vj_cascade* c = nullptr;
        if (vj_cascade_load_xml(xpath.c_str(), &c) != VJ_OK) { fprintf(stderr, "embedded XML refused: %s\n", vj_last_error()); return 1; }
        vj_cascade_info info;
        vj_cascade_get_info(c, &info);
        if (info.n_stages != 2 || info.n_trees != 3 || info.n_nodes != 4 || info.n_tilted != 1 || info.max_nodes_per_tree != 2) return 1;
        exercise(c);
        {   // its tilted node: planned as upright only on request
            vj_params p;
            vj_params_default(&p);
            int n = 0;
            if (vj_plan_tiles(c, 320, 240, &p, 1, 0, nullptr, nullptr, 0, &n) != VJ_ERR_UNSUPPORTED || !strstr(vj_last_error(), "tilted")) return 1;
        }
        vj_cascade_free(c);
    }
    {   // the same cascade with a tilted rectangle whose corner (x - h, y + h) lies left of the window: refused at load
        std::string out = xml;
        const std::string legal = "<_>9 2 9 9 -1.</_>";
        out.replace(out.find(legal), legal.size(), "<_>1 7 15 9 -1.</_>");
        spit(xpath, out);
        vj_cascade* c = nullptr;
        const int rc = vj_cascade_load_xml(xpath.c_str(), &c);
        if (rc != VJ_ERR_PARSE || c != nullptr || !strstr(vj_last_error(), "node 2 rect 0")) {
            fprintf(stderr, "a tilted rectangle outside the window was not refused (%d: %s)\n", rc, vj_last_error());
            return 1;
        }
    }
    for (size_t len = 0; len < xml.size(); len += 3) {
        spit(xpath, xml.substr(0, len));
        vj_cascade* c = nullptr;
        if (vj_cascade_load_xml(xpath.c_str(), &c) == VJ_OK) vj_cascade_free(c);
    }
    const char* junk[] = {"<", ">", "</_>", "<_>", "-1", "99999999999", "1e999", "<!--", "-->", "&amp;", "\0", "<trees>", "nan", "<rects></rects>"};
    for (int trial = 0; trial < 600; ++trial) {
        std::string m = xml;
        const int edits = 1 + (int)(rnd() % 4);
        for (int k = 0; k < edits; ++k) {
            const size_t pos = rnd() % m.size();
            switch (rnd() % 3) {
                case 0: m.erase(pos, 1 + rnd() % 20); break;
                case 1: m.insert(pos, junk[rnd() % (sizeof(junk) / sizeof(junk[0]))]); break;
                default: m[pos] = (char)(32 + rnd() % 95); break;
            }
            if (m.empty()) m = "x";
        }
        spit(xpath, m);
        vj_cascade* c = nullptr;
        if (vj_cascade_load_xml(xpath.c_str(), &c) == VJ_OK) {
            exercise(c);
            vj_cascade_free(c);
            ++loaded;
        } else {
            ++refused;
        }
    }
    // 4. in-memory arrays of garbage
    for (int trial = 0; trial < 300; ++trial) {
        const int ns = 1 + (int)(rnd() % 4), nt = 1 + (int)(rnd() % 6), nn = 1 + (int)(rnd() % 9), na = 1 + (int)(rnd() % 12);
        std::vector<vj_stage_desc> st((size_t)ns);
        std::vector<vj_tree_desc> tr((size_t)nt);
        std::vector<vj_node_desc> nd((size_t)nn);
        std::vector<float> al((size_t)na, 0.5f);
        auto small = [&]() { return (int32_t)(rnd() % 9) - 2; };
        for (auto& s : st) s = vj_stage_desc{small(), small(), 0.5f, small(), small(), small()};
        for (auto& t : tr) t = vj_tree_desc{small(), small(), small()};
        for (auto& n : nd) {
            memset(&n, 0, sizeof(n));
            n.n_rects = small();
            n.left = small();
            n.right = small();
            for (auto& r : n.rect) r = vj_rect_desc{small(), small(), small() * 3, small() * 3, (float)small()};
        }
        vj_cascade* c = nullptr;
        if (vj_cascade_from_arrays(20, 20, st.data(), ns, tr.data(), nt, nd.data(), nn, al.data(), na, &c) == VJ_OK) {
            exercise(c);
            vj_cascade_free(c);
            ++loaded;
        } else {
            ++refused;
        }
    }
    // 5. rectangle grouping on degenerate lists
    for (int trial = 0; trial < 200; ++trial) {
        const uint32_t n0 = rnd() % 200;
        std::vector<vj_rect> r(n0 ? n0 : 1);
        int frame = 0;
        for (uint32_t i = 0; i < n0; ++i) {
            if (rnd() % 16 == 0) ++frame;
            const int big = trial % 5 == 0 ? 1 << 20 : 400;
            r[i] = vj_rect{(int32_t)(rnd() % big), (int32_t)(rnd() % big), (int32_t)(rnd() % 90), (int32_t)(rnd() % 90), 0.0f, frame, (int32_t)(rnd() % 40)};
            if (trial % 7 == 0 && i) r[i] = r[0], r[i].frame = frame;
        }
        uint32_t n = n0;
        if (vj_group_rectangles(n0 ? r.data() : nullptr, &n, (int)(rnd() % 4), 0.2) != VJ_OK || n > n0) { fprintf(stderr, "grouping failed\n"); return 1; }
    }
    {   // rectangles that are no image rectangles are refused, not summed
        vj_rect r = {1 << 28, 0, 10, 10, 0.0f, 0, 0};
        uint32_t n = 1;
        if (vj_group_rectangles(&r, &n, 1, 0.2) != VJ_ERR_ARG) return 1;
    }
    if (plans_ok == 0) { fprintf(stderr, "no plan query gave a plan\n"); return 1; }
    printf("host_asan_driver: OK (%d cascades accepted, %d inputs refused; %d plan queries gave a plan, %d an error code; OpenCV-profile plans per "
           "mode %d %d %d %d %d, %d error codes)\n",
           loaded, refused, plans_ok, plans_refused, cv_plans_ok[0], cv_plans_ok[1], cv_plans_ok[2], cv_plans_ok[3], cv_plans_ok[4], cv_plans_refused);
    return 0;
}
