// Miss links of the stackless walk (crt_device.hip walk(), LINK): the one definition of the table,
// its builder and its validator. Host code only, with no dependency but the node layout, so that
// crt_host.cpp (every upload, crt_walk_links) and tools/walk_links_check.cpp (the same functions
// under a sanitizer) compile the same text.
//
// BVH::hit_by (bvh.h:684-698) takes the near child by dir_is_negative[split_axis] alone, so the
// DFS order of a ray is fixed by its three sign bits: the octant, Trav::neg bits 0-2. The node a
// pop returns is therefore a function of (node, octant):
//   miss(root, o) = the sentinel;
//   for an interior node N with near child n and far child f under o:
//   miss(n, o) = f, miss(f, o) = miss(N, o).
// Table: 8 u16 entries per device node, entry o = miss(node, o) as a node ref (the byte offset of
// the f32 node, index << kNodeFShift), 16 bytes a node, so the record of ref r sits at byte r >> 1.
// The sentinel's links (and those of the pad, node 1, which no node refers to) are the sentinel.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "crt_internal.h"

namespace crt {

constexpr size_t kWalkLinkOctants = 8;
// every ref fits a u16 entry (the walk's own entry width for LDS scenes)
inline bool walk_links_fit(size_t num_nodes) { return num_nodes >= 2 && (num_nodes << kNodeFShift) <= 65536; }

// node_record's classes
inline bool walk_node_interior(const DevNode& n) { return n.count == 0 && n.index == n.flags + 1 && !(n.flags & 1u); }

// Builds the table for `n` device nodes (the last one the sentinel), top-down in one pass: a
// node's links are final before its children's are derived from them, which needs every parent
// before its children in device order. False (table unusable) when that does not hold, a child
// index is out of range or has two parents, or the array does not end with the sentinel.
inline bool build_walk_links(const DevNode* nodes, size_t n, std::vector<uint16_t>& links) {
    links.clear();
    if (!walk_links_fit(n) || nodes[n - 1].count != kSentinelCount) return false;
    const uint16_t sentinel = static_cast<uint16_t>((n - 1) << kNodeFShift);
    links.assign(n * kWalkLinkOctants, sentinel);
    std::vector<unsigned char> placed(n, 0);
    placed[0] = 1;  // the root: miss = the sentinel
    for (size_t i = 0; i + 1 < n; ++i) {
        const DevNode& nd = nodes[i];
        if (!walk_node_interior(nd)) continue;
        if (!placed[i]) {
            if (i == 1) continue;  // the pad is a leaf; an interior node nobody refers to is malformed
            return false;
        }
        const size_t left = nd.flags, right = nd.index;
        if (left <= i || right >= n - 1 || nd.axis > 2 || placed[left] || placed[right]) return false;
        placed[left] = placed[right] = 1;
        for (size_t o = 0; o < kWalkLinkOctants; ++o) {
            const bool far_first = (o >> nd.axis) & 1u;  // children: left = flags, right = index
            const size_t near = far_first ? right : left, far = far_first ? left : right;
            links[near * kWalkLinkOctants + o] = static_cast<uint16_t>(far << kNodeFShift);
            links[far * kWalkLinkOctants + o] = links[i * kWalkLinkOctants + o];
        }
    }
    return true;
}

// Checks a table against the tree alone (not against the builder): under each octant the link of a
// node must be the node that follows its subtree in that octant's DFS order (the sentinel after the
// last one), which puts every link later in the order; and following links from any node must
// reach the sentinel within n steps. A wrong link is an endless loop of a wave, so a table that
// fails is dropped and the scene keeps the stack walk.
inline bool validate_walk_links(const DevNode* nodes, size_t n, const uint16_t* links) {
    if (!walk_links_fit(n) || nodes[n - 1].count != kSentinelCount) return false;
    const size_t sentinel = n - 1;
    std::vector<uint32_t> order, rank(n), size(n), stack;
    for (size_t o = 0; o < kWalkLinkOctants; ++o) {
        // the octant's DFS order, near child first, with an explicit stack; a node met twice or
        // more nodes than the array holds is a malformed tree
        order.clear();
        stack.assign(1, 0u);
        std::vector<unsigned char> seen(n, 0);
        while (!stack.empty()) {
            const uint32_t i = stack.back();
            stack.pop_back();
            if (i >= sentinel || seen[i]) return false;
            seen[i] = 1;
            rank[i] = static_cast<uint32_t>(order.size());
            order.push_back(i);
            const DevNode& nd = nodes[i];
            if (!walk_node_interior(nd)) continue;
            if (nd.axis > 2) return false;
            const bool far_first = (o >> nd.axis) & 1u;
            stack.push_back(far_first ? nd.flags : nd.index);  // the far child, popped second
            stack.push_back(far_first ? nd.index : nd.flags);
        }
        // subtree sizes, children after parents in the order
        for (size_t k = order.size(); k-- > 0;) {
            const uint32_t i = order[k];
            size[i] = 1;
            if (walk_node_interior(nodes[i])) size[i] += size[nodes[i].flags] + size[nodes[i].index];
        }
        for (size_t i = 0; i < n; ++i) {
            const size_t link = links[i * kWalkLinkOctants + o];
            if (link & ((size_t{1} << kNodeFShift) - 1)) return false;
            const size_t t = link >> kNodeFShift;
            if (t >= n) return false;
            if (i == sentinel || !seen[i]) {  // the sentinel, the pad
                if (t != sentinel) return false;
                continue;
            }
            const size_t after = static_cast<size_t>(rank[i]) + size[i];
            const size_t want = after < order.size() ? order[after] : sentinel;
            if (t != want) return false;
            if (t != sentinel && rank[t] <= rank[i]) return false;
        }
        for (size_t i = 0; i < n; ++i) {
            size_t cur = i, steps = 0;
            while (cur != sentinel) {
                if (++steps > n) return false;
                cur = links[cur * kWalkLinkOctants + o] >> kNodeFShift;
            }
        }
    }
    return true;
}

}  // namespace crt
