// Host planner of the mixed-size entry points that needs no device: see vj_atlas_host.hpp.
#include "vj_atlas_host.hpp"

#include <algorithm>
#include <cmath>
#include <map>
#include <numeric>
#include <tuple>

namespace vj {

namespace {
inline uint32_t align4(uint32_t v) { return (v + 3u) & ~3u; }
}  // namespace

uint32_t atlas_ladder(uint32_t v) {
    v = std::max(v, 1u);
    uint32_t p2 = 1;
    while (p2 <= v / 2u) p2 *= 2u;
    const uint64_t q = std::max(32u, p2 / 4u);
    return (uint32_t)std::min<uint64_t>(((uint64_t)v + q - 1u) / q * q, 0xffffffe0ull);
}

int atlas_check_frames(const vj_image* frames, int n_frames, std::vector<AtlasSize>* sizes) {
    sizes->clear();
    if (n_frames < 0 || (n_frames > 0 && !frames)) return VJ_ERR_ARG;
    sizes->reserve((size_t)n_frames);
    for (int i = 0; i < n_frames; ++i) {
        const vj_image& f = frames[i];
        const int ch = f.channels <= 1 ? 1 : f.channels;
        if (!f.data || f.width <= 0 || f.height <= 0 || (ch != 1 && ch != 3 && ch != 4) || (int64_t)f.stride < (int64_t)f.width * ch) {
            set_error("frame %d: %s", i, !f.data ? "null data" : f.width <= 0 || f.height <= 0 ? "width and height must be positive"
                                         : (ch != 1 && ch != 3 && ch != 4) ? "frames must have 1 (gray), 3 (BGR) or 4 (BGRA) channels"
                                                                           : "stride is below width * channels");
            return VJ_ERR_ARG;
        }
        sizes->push_back(AtlasSize{f.width, f.height, ch});
    }
    return VJ_OK;
}

std::vector<std::vector<int>> atlas_size_groups(const std::vector<AtlasSize>& sizes, const std::vector<int>& idx) {
    std::map<std::tuple<int, int, int>, std::vector<int>> by_size;
    for (int i : idx) by_size[std::make_tuple(sizes[(size_t)i].w, sizes[(size_t)i].h, sizes[(size_t)i].ch)].push_back(i);
    std::vector<std::vector<int>> groups;
    groups.reserve(by_size.size());
    for (auto& kv : by_size) groups.push_back(std::move(kv.second));
    return groups;
}

AtlasRoute atlas_route(const std::vector<AtlasSize>& sizes, uint64_t own_call_px, bool all_own) {
    AtlasRoute r;
    std::vector<int> every(sizes.size());
    std::iota(every.begin(), every.end(), 0);
    for (std::vector<int>& g : atlas_size_groups(sizes, every)) {
        const AtlasSize& s = sizes[(size_t)g[0]];
        const uint64_t px = (uint64_t)s.w * (uint64_t)s.h * (uint64_t)g.size();
        if (all_own || px >= own_call_px) r.own.push_back(std::move(g));
        else r.packed.insert(r.packed.end(), g.begin(), g.end());
    }
    std::sort(r.packed.begin(), r.packed.end());
    return r;
}

namespace {

// Shelves of the atlas's width, tallest frame first: one goes to the first shelf with room beside what it holds (every shelf is at
// least as high as anything that comes after it), else it opens a new shelf below.  false: the slots exceed the budget, or the atlas
// the 32-bit offsets of a frame's sum image.
bool pack_shelves(const std::vector<AtlasSize>& sizes, const std::vector<int>& order, size_t first, size_t n, uint64_t budget_px,
                  std::vector<uint32_t>* ox, std::vector<uint32_t>* oy, uint32_t* aw_, uint32_t* ah_) {
    uint64_t area = 0;
    uint32_t widest = 4;
    for (size_t i = 0; i < n; ++i) {
        const AtlasSize& s = sizes[(size_t)order[first + i]];
        area += (uint64_t)align4((uint32_t)s.w) * (uint64_t)s.h;
        widest = std::max(widest, align4((uint32_t)s.w));
    }
    if (area > budget_px || widest > (1u << 30)) return false;
    const uint32_t W = atlas_ladder(std::max(widest, align4((uint32_t)std::ceil(std::sqrt((double)area)))));
    std::vector<size_t> by_height(n);
    std::iota(by_height.begin(), by_height.end(), (size_t)0);
    std::stable_sort(by_height.begin(), by_height.end(),
                     [&](size_t x, size_t y) { return sizes[(size_t)order[first + x]].h > sizes[(size_t)order[first + y]].h; });
    struct Shelf { uint32_t y, used; };
    std::vector<Shelf> shelves;
    size_t open = 0;   // shelves before this one are full to within one slot of the narrowest kind: not searched again
    uint64_t H = 0;
    ox->assign(n, 0u);
    oy->assign(n, 0u);
    for (size_t i : by_height) {
        const AtlasSize& s = sizes[(size_t)order[first + i]];
        const uint32_t aw = align4((uint32_t)s.w);
        Shelf* fit = nullptr;
        for (size_t k = open; k < shelves.size(); ++k)
            if (shelves[k].used + aw <= W) { fit = &shelves[k]; break; }
        if (!fit) {
            shelves.push_back(Shelf{(uint32_t)H, 0u});
            H += (uint64_t)s.h;
            fit = &shelves.back();
        }
        (*ox)[i] = fit->used;
        (*oy)[i] = fit->y;
        fit->used += aw;
        while (open < shelves.size() && shelves[open].used + 4u > W) ++open;
    }
    if (H >= 65535ull) return false;
    H = atlas_ladder((uint32_t)std::max<uint64_t>(H, 1));
    if (H >= 65535ull || (uint64_t)(W + 1u) * (H + 3ull) >= (1ull << 30)) return false;
    *aw_ = W;
    *ah_ = (uint32_t)H;
    return true;
}

}  // namespace

int atlas_plan(const std::vector<AtlasSize>& sizes, const std::vector<int>& order, size_t first, uint64_t budget_px, int max_frames,
               AtlasPlan* out) {
    *out = AtlasPlan{};
    if (first >= order.size()) return VJ_OK;
    // ---- the frames from `first` on, while their slots stay within the budget (the first one in any case)
    size_t take = 0;
    uint64_t area = 0;
    for (size_t r = first; r < order.size(); ++r) {
        const int f = order[r];
        if (f < 0 || (size_t)f >= sizes.size() || sizes[(size_t)f].w <= 0 || sizes[(size_t)f].h <= 0) {
            set_error("frame %d is not an image", f);
            return VJ_ERR_ARG;
        }
        const uint64_t a = (uint64_t)align4((uint32_t)std::min(sizes[(size_t)f].w, 1 << 30)) * (uint64_t)sizes[(size_t)f].h;
        if (r > first && (area + a > budget_px || (max_frames > 0 && take >= (size_t)max_frames))) break;
        area += a;
        ++take;
    }
    // ---- pack; an atlas the shelves and the ladder make larger than the 32-bit offsets allow takes fewer frames
    std::vector<uint32_t> ox, oy;
    uint32_t aw = 0, ah = 0;
    while (take > 0 && !pack_shelves(sizes, order, first, take, budget_px, &ox, &oy, &aw, &ah)) take = take == 1 ? 0 : std::max<size_t>(1, take * 3 / 4);
    if (take == 0) {
        out->oversized = true;
        out->n_frames = 1;
        return VJ_OK;
    }
    out->n_frames = take;
    out->w = aw;
    out->h = ah;
    out->pitch = aw;
    out->slots.resize(take);
    uint64_t unit = 0;
    for (size_t i = 0; i < take; ++i) {
        const AtlasSize& s = sizes[(size_t)order[first + i]];
        out->slots[i] = AtlasSlot{order[first + i], ox[i], oy[i], (uint32_t)s.w, (uint32_t)s.h, (uint32_t)unit};
        unit += (uint64_t)(((uint32_t)s.w + ATLAS_BLOCK_W - 1u) / ATLAS_BLOCK_W) * (uint64_t)(((uint32_t)s.h + ATLAS_BLOCK_H - 1u) / ATLAS_BLOCK_H);
        if (unit > 0x7fffffffull) {   // (cannot happen within the offset limit above: an atlas holds fewer units than pixels)
            set_error("the frames of an atlas hold more pack units than a 32-bit index holds");
            return VJ_ERR_LIMIT;
        }
    }
    out->n_units = (uint32_t)unit;
    return VJ_OK;
}

}  // namespace vj
