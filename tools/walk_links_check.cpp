// The miss-link builder and validator of the stackless walk (cpp_raytracer_amd/csrc/crt_walk_links.h)
// as a stand-alone host program, for a sanitizer build: the same text crt_host.cpp compiles, fed random
// trees in the device node order (root, pad, sibling pairs, sentinel), a root that is a leaf, one
// interior node, degenerate chains up to the u16 limit and malformed arrays. Every built table must
// validate, equal the recursive definition, and stop validating with any one entry changed.
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I cpp_raytracer_amd/csrc tools/walk_links_check.cpp -o tools/build/walk_links_check
//   tools/build/walk_links_check [small random trees, default 10000]
//                                       (prints "walk links ok: ..." and exits 0)
// Host only: it is never loaded into Python and never runs on a GPU.
// tests/test_walk_links_sanitized.py builds it this way and runs it as a child program.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <vector>

#include "crt_walk_links.h"

using namespace crt;

static void fail_at(const char* what, size_t tree) {
    std::fprintf(stderr, "walk links FAILED: %s (tree %zu)\n", what, tree);
    std::exit(1);
}

struct Tree {
    std::vector<DevNode> nodes;  // device order, the sentinel last
};

// a random tree of `leaves` leaves: split a random leaf until enough; side < 2 makes a chain
static Tree make_tree(std::mt19937& rng, size_t leaves, int side) {
    Tree t;
    t.nodes.resize(2);
    auto leaf = [](DevNode& n) {
        n = DevNode{};
        n.count = 1;
    };
    leaf(t.nodes[0]);
    leaf(t.nodes[1]);  // the pad
    std::vector<uint32_t> open{0};
    for (size_t k = 1; k < leaves; ++k) {
        const size_t pick = side < 2 ? open.size() - 1 : rng() % open.size();
        const uint32_t i = open[pick];
        open.erase(open.begin() + static_cast<long>(pick));
        const uint32_t l = static_cast<uint32_t>(t.nodes.size());
        t.nodes.resize(l + 2);
        leaf(t.nodes[l]);
        leaf(t.nodes[l + 1]);
        DevNode& n = t.nodes[i];
        n.count = 0;
        n.flags = l;
        n.index = l + 1;
        n.axis = rng() % 3;
        if (side == 0) {
            open.push_back(l + 1);
            open.push_back(l);
        } else {
            open.push_back(l);
            open.push_back(l + 1);
        }
    }
    DevNode z{};
    z.count = kSentinelCount;
    z.index = z.flags = static_cast<uint32_t>(t.nodes.size());
    t.nodes.push_back(z);
    return t;
}

int main(int argc, char** argv) {
    const int random_trees = argc > 1 ? std::atoi(argv[1]) : 10000;  // small random trees (default 10000)
    std::mt19937 rng(20260107u);
    size_t trees = 0, corruptions = 0;
    std::vector<uint16_t> links;
    auto check = [&](const Tree& t) {
        const size_t n = t.nodes.size();
        if (!build_walk_links(t.nodes.data(), n, links)) fail_at("build refused a good tree", trees);
        if (links.size() != n * kWalkLinkOctants) fail_at("table size", trees);
        if (!validate_walk_links(t.nodes.data(), n, links.data())) fail_at("a built table did not validate", trees);
        // the recursive definition
        std::vector<uint16_t> want(n * 8, static_cast<uint16_t>((n - 1) << kNodeFShift));
        std::function<void(size_t)> down = [&](size_t i) {
            const DevNode& nd = t.nodes[i];
            if (!walk_node_interior(nd)) return;
            for (size_t o = 0; o < 8; ++o) {
                const bool ff = (o >> nd.axis) & 1u;
                const size_t near = ff ? nd.index : nd.flags, far = ff ? nd.flags : nd.index;
                want[near * 8 + o] = static_cast<uint16_t>(far << kNodeFShift);
                want[far * 8 + o] = want[i * 8 + o];
            }
            down(nd.flags);
            down(nd.index);
        };
        down(0);
        if (want != links) fail_at("the table is not the recursive definition's", trees);
        // one entry changed
        for (int k = 0; k < 8 && n > 3; ++k) {
            size_t i = rng() % (n - 1);
            if (i == 1) i = 0;
            const size_t o = rng() % 8;
            uint16_t bad = static_cast<uint16_t>((rng() % n) << kNodeFShift);
            if (k == 0) bad = static_cast<uint16_t>(i << kNodeFShift);  // itself: the endless loop
            if (k == 1) bad = static_cast<uint16_t>(links[i * 8 + o] + 2);
            if (bad == links[i * 8 + o]) continue;
            std::vector<uint16_t> c = links;
            c[i * 8 + o] = bad;
            if (validate_walk_links(t.nodes.data(), n, c.data())) fail_at("a corrupted table validated", trees);
            ++corruptions;
        }
        ++trees;
    };
    check(make_tree(rng, 1, 2));  // the root is a leaf
    check(make_tree(rng, 2, 2));  // one interior node
    for (int side = 0; side < 2; ++side)
        for (size_t leaves : {3u, 17u, 200u, 1022u}) check(make_tree(rng, leaves, side));  // chains; 2047 nodes at most
    for (int k = 0; k < random_trees; ++k) check(make_tree(rng, 1 + rng() % 64, 2));
    for (int k = 0; k < 50; ++k) check(make_tree(rng, 1 + rng() % 1022, 2));
    // arrays the builder must refuse: beyond u16 references, no sentinel, a child before its parent, a
    // child out of range, a node with two parents
    {
        Tree t = make_tree(rng, 1024, 2);  // 2049 nodes
        if (build_walk_links(t.nodes.data(), t.nodes.size(), links) || !links.empty()) fail_at("built beyond u16", trees);
        if (validate_walk_links(t.nodes.data(), t.nodes.size(), std::vector<uint16_t>(t.nodes.size() * 8).data()))
            fail_at("validated beyond u16", trees);
        t = make_tree(rng, 9, 2);
        t.nodes.back().count = 1;
        if (build_walk_links(t.nodes.data(), t.nodes.size(), links)) fail_at("built without a sentinel", trees);
        t = make_tree(rng, 9, 2);
        const std::vector<DevNode> good = t.nodes;
        for (int bad = 0; bad < 3; ++bad) {
            t.nodes = good;
            for (size_t i = 2; i + 1 < t.nodes.size(); ++i) {
                DevNode& nd = t.nodes[i];
                if (!walk_node_interior(nd)) continue;
                if (bad == 0) nd.flags = 0, nd.index = 1;                                           // before its parent
                if (bad == 1) nd.flags = static_cast<uint32_t>(t.nodes.size()), nd.index = nd.flags + 1;  // out of range
                if (bad == 2) nd.flags = t.nodes[0].flags, nd.index = nd.flags + 1;                     // the root's children again
                break;
            }
            if (build_walk_links(t.nodes.data(), t.nodes.size(), links)) fail_at("built a malformed tree", static_cast<size_t>(bad));
            build_walk_links(good.data(), good.size(), links);
            if (validate_walk_links(t.nodes.data(), t.nodes.size(), links.data())) fail_at("validated a malformed tree", static_cast<size_t>(bad));
        }
    }
    std::printf("walk links ok: %zu trees, %zu corrupted tables refused\n", trees, corruptions);
    return 0;
}
