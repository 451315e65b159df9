// Host self-test of cuda-slam_amd/csrc/voxel_table.hpp, the voxel hash table of the NDT map, the TSDF map and the ray cast's skip blocks:
// this file includes the header alone, no HIP, and is built as a program of its own, plain and under the address and undefined-behaviour
// sanitizers (tests/test_voxel_table.py), with -ffp-contract=off as the library is.  The claiming probe is the loop the kernels run, with a
// plain compare-and-set where they have a compare-and-swap.  Without arguments it checks facts with known answers.  With `in out` it reads
// a list of voxel coordinates and some orders of insertion from `in` (the layout below, written by the test), builds the table once per
// order and writes every row's key and hash, and per order every row's slot and the row found for every cell of the listed box, to `out`.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../cuda-slam_amd/csrc/voxel_table.hpp"

using namespace mislam;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

struct HostTable {
    std::vector<unsigned long long> keys;
    std::vector<int> vals;
    VoxelTableView view;
};

static unsigned long long row_key(const VoxelTableView& t, const int32_t* c) { return voxel_key(c[0] - t.cmin[0], c[1] - t.cmin[1], c[2] - t.cmin[2]); }

// the table of the rows of coord (nv x 3), inserted in `order`, at `per` slots per row; slot_of: the slot every row got.  false: a row
// found no slot, or was met twice
static bool build(const std::vector<int32_t>& coord, const std::vector<int32_t>& order, unsigned long long per, HostTable* t, std::vector<long long>* slot_of)
{
    const size_t nv = coord.size() / 3;
    int cmin[3], cmax[3];
    for (int a = 0; a < 3; a++) cmin[a] = cmax[a] = coord[a];
    for (size_t i = 0; i < nv; i++)
        for (int a = 0; a < 3; a++) {
            if (coord[3 * i + a] < cmin[a]) cmin[a] = coord[3 * i + a];
            if (coord[3 * i + a] > cmax[a]) cmax[a] = coord[3 * i + a];
        }
    t->view = VoxelTableView{};
    if (voxel_table_frame(&t->view, cmin, cmax) >= 0) return false;
    const unsigned long long slots = voxel_table_slots(nv, per);
    if (!voxel_table_holds(slots - 1, nv, per)) return false;
    t->keys.assign((size_t)slots, VOXEL_KEY_EMPTY);
    t->vals.assign((size_t)slots, -7);
    voxel_table_bind(&t->view, t->keys.data(), t->vals.data(), slots);
    slot_of->assign(nv, -1);
    for (int32_t row : order) {
        bool fresh = false;
        const long long slot = voxel_claim(t->keys.data(), t->view.mask, row_key(t->view, &coord[3 * (size_t)row]), &fresh);
        if (slot < 0 || !fresh) return false;
        t->vals[(size_t)slot] = row;
        (*slot_of)[(size_t)row] = slot;
    }
    return true;
}

static int run_file(const char* in, const char* out)
{
    std::FILE* f = std::fopen(in, "rb");
    if (!f) { std::printf("cannot read %s\n", in); return 2; }
    int32_t head[2] = {0, 0};                // nv, orders; then nv x 3 int32 coordinates and orders x nv int32 rows
    bool ok = std::fread(head, sizeof head, 1, f) == 1 && head[0] >= 1 && head[1] >= 1;
    std::vector<int32_t> coord(ok ? 3 * (size_t)head[0] : 0), orders(ok ? (size_t)head[0] * (size_t)head[1] : 0);
    ok = ok && std::fread(coord.data(), sizeof(int32_t), coord.size(), f) == coord.size() && std::fread(orders.data(), sizeof(int32_t), orders.size(), f) == orders.size();
    std::fclose(f);
    if (!ok) { std::printf("short input %s\n", in); return 2; }
    const size_t nv = (size_t)head[0];
    for (int32_t row : orders)
        if (row < 0 || (size_t)row >= nv) { std::printf("a row outside the list\n"); return 2; }

    std::FILE* g = std::fopen(out, "wb");
    if (!g) { std::printf("cannot write %s\n", out); return 2; }
    for (int32_t o = 0; o < head[1]; o++) {
        const std::vector<int32_t> order(orders.begin() + (size_t)o * nv, orders.begin() + (size_t)(o + 1) * nv);
        HostTable t;
        std::vector<long long> slot_of;
        if (!build(coord, order, 2, &t, &slot_of)) { std::printf("order %d: the table was not built\n", o); std::fclose(g); return 1; }
        const int* e = t.view.ext;
        if (o == 0) {                        // slots, cells of the box, then every row's key and hash
            const unsigned long long dims[2] = {t.view.mask + 1, (unsigned long long)e[0] * e[1] * e[2]};
            std::vector<unsigned long long> keys(nv), hashes(nv);
            for (size_t i = 0; i < nv; i++) { keys[i] = row_key(t.view, &coord[3 * i]); hashes[i] = voxel_hash(keys[i]); }
            std::fwrite(dims, sizeof dims, 1, g);
            std::fwrite(keys.data(), sizeof(unsigned long long), nv, g);
            std::fwrite(hashes.data(), sizeof(unsigned long long), nv, g);
        }
        VoxelTableView keys_only = t.view;
        keys_only.vals = nullptr;
        std::vector<int32_t> found;          // every cell of the box, x fastest
        for (int z = 0; z < e[2]; z++)
            for (int y = 0; y < e[1]; y++)
                for (int x = 0; x < e[0]; x++) {
                    const int c[3] = {t.view.cmin[0] + x, t.view.cmin[1] + y, t.view.cmin[2] + z};
                    found.push_back(voxel_row(t.view, c[0], c[1], c[2]));
                    CHECK(voxel_present(keys_only, c[0], c[1], c[2]) == (found.back() >= 0));
                }
        std::fwrite(slot_of.data(), sizeof(long long), nv, g);
        std::fwrite(found.data(), sizeof(int32_t), found.size(), g);
    }
    std::fclose(g);
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc == 3) return run_file(argv[1], argv[2]);

    // sizing: 2 slots per key for the maps, 54 for the dilated block table; what a launch wrapper admits
    {
        const unsigned long long nv[7] = {1, 2, 3, 4, 5, 1024, 1025}, slots[7] = {2, 4, 8, 8, 16, 2048, 4096};
        for (int i = 0; i < 7; i++) CHECK(voxel_table_slots(nv[i], 2) == slots[i] && voxel_table_holds(slots[i] - 1, nv[i], 2) && !voxel_table_holds(slots[i] / 2 - 1, nv[i], 2));
        CHECK(voxel_table_slots(1, 54) == 64 && voxel_table_slots(2, 54) == 128 && voxel_table_slots(18, 54) == 1024 && voxel_table_slots(19, 54) == 2048);
        CHECK(voxel_table_holds(63, 1, 54) && !voxel_table_holds(31, 1, 54) && !voxel_table_holds(62, 1, 54) && !voxel_table_holds(64, 1, 54));
        CHECK(!voxel_table_holds(~0ull, 1, 2));                  // (mask + 1 wraps to 0)
    }
    // constants, hash, key
    CHECK(VOXEL_KEY_EMPTY == ~0ull && VOXEL_KEY_BITS == 20 && VOXEL_MAX_EXTENT == 1048576);
    CHECK(voxel_hash(0x9e3779b97f4a7c15ull) == 0xe220a8397b1dcdafull && voxel_hash(0) == 0);      // splitmix64 from the state 0: its first output
    {
        const int top = (1 << 20) - 1;
        CHECK(voxel_key(0, 0, 0) == 0 && voxel_key(1, 0, 0) == 1 && voxel_key(0, 1, 0) == 1ull << 20 && voxel_key(0, 0, 1) == 1ull << 40);
        CHECK(voxel_key(top, top, top) == (1ull << 60) - 1 && voxel_key(top, top, top) != VOXEL_KEY_EMPTY);
        const int cases[5][3] = {{0, 0, 0}, {top, 0, 0}, {0, top, 0}, {0, 0, top}, {top, top, top}};
        for (const int* c : cases) {
            const unsigned long long key = voxel_key(c[0], c[1], c[2]);
            CHECK(voxel_key_axis(key, 0) == c[0] && voxel_key_axis(key, 1) == c[1] && voxel_key_axis(key, 2) == c[2]);
        }
    }
    // the frame of a list, and the keys inside it
    {
        const int cmin[3] = {5, -2, 7}, cmax[3] = {6, -1, 8};
        VoxelTableView t{};
        CHECK(voxel_table_frame(&t, cmin, cmax) == -1 && t.cmin[0] == 5 && t.cmin[1] == -2 && t.cmin[2] == 7 && t.ext[0] == 2 && t.ext[1] == 2 && t.ext[2] == 2);
        unsigned long long k[4] = {9, 9, 9, 9};
        CHECK(voxel_key_in_frame(t, 5, -2, 7, &k[0]) && voxel_key_in_frame(t, 6, -2, 7, &k[1]) && voxel_key_in_frame(t, 5, -1, 7, &k[2]) && voxel_key_in_frame(t, 5, -2, 8, &k[3]));
        CHECK(k[0] == 0 && k[1] == 1 && k[2] == 1ull << 20 && k[3] == 1ull << 40);
        const int low = -(1 << 30), wide[3] = {low + (1 << 20) - 1, low, low + 4}, wider[3] = {low + (1 << 20), low, low}, lows[3] = {low, low, low}, under[3] = {low, low - 1, low};
        CHECK(voxel_table_frame(&t, lows, wide) == -1 && t.ext[0] == 1 << 20 && t.ext[1] == 1 && t.ext[2] == 5);      // the limit itself, admitted
        VoxelTableView u{};
        CHECK(voxel_table_frame(&u, lows, wider) == 0 && voxel_extent(lows, wider, 0) == (1ll << 20) + 1 && voxel_table_frame(&u, lows, under) == 1);
        const int all_lo[3] = {-2147483647 - 1, 0, 0}, all_hi[3] = {2147483647, 0, 0};
        CHECK(voxel_table_frame(&u, all_lo, all_hi) == 0 && voxel_extent(all_lo, all_hi, 0) == 1ll << 32);
        // both faces on every axis, with cmin = -2^30: one inside, one outside; the differences do not wrap in 32 bits
        unsigned long long key = 9;
        CHECK(voxel_key_in_frame(t, low, low, low, &key) && key == 0);
        CHECK(voxel_key_in_frame(t, wide[0], low, low + 4, &key) && key == (((1ull << 20) - 1) | 4ull << 40));
        CHECK(!voxel_key_in_frame(t, low - 1, low, low, &key) && !voxel_key_in_frame(t, wide[0] + 1, low, low, &key));
        CHECK(!voxel_key_in_frame(t, low, low - 1, low, &key) && !voxel_key_in_frame(t, low, low + 1, low, &key));
        CHECK(!voxel_key_in_frame(t, low, low, low - 1, &key) && !voxel_key_in_frame(t, low, low, low + 5, &key));
        CHECK(!voxel_key_in_frame(t, (1 << 30) - 1, low, low, &key) && !voxel_key_in_frame(t, low, 2147483647, low, &key) && !voxel_key_in_frame(t, low, low, -2147483647 - 1, &key));
        CHECK(key == (((1ull << 20) - 1) | 4ull << 40));          // a refusal forms no key
    }
    // a key-only table: new, then not new; present and absent; a full table refuses and ends
    {
        std::vector<unsigned long long> keys(8, VOXEL_KEY_EMPTY);
        bool fresh = false;
        const long long s = voxel_claim(keys.data(), 7, voxel_key(3, 2, 1), &fresh);
        CHECK(s >= 0 && s == (long long)(voxel_hash(voxel_key(3, 2, 1)) & 7) && fresh && keys[(size_t)s] == voxel_key(3, 2, 1));
        CHECK(voxel_claim(keys.data(), 7, voxel_key(3, 2, 1), &fresh) == s && !fresh && voxel_claim(keys.data(), 7, voxel_key(3, 2, 1)) == s);
        VoxelTableView t{};
        voxel_table_bind(&t, keys.data(), nullptr, 8);
        t.ext[0] = t.ext[1] = t.ext[2] = 4;
        CHECK(t.mask == 7 && voxel_present(t, 3, 2, 1) && !voxel_present(t, 1, 2, 3) && !voxel_present(t, 4, 2, 1) && !voxel_present(t, 3, 2, -1));
        std::vector<unsigned long long> full = {voxel_key(1, 0, 0), voxel_key(2, 0, 0)};
        fresh = true;
        CHECK(voxel_claim(full.data(), 1, voxel_key(3, 0, 0), &fresh) == -1 && !fresh && voxel_find(full.data(), 1, voxel_key(3, 0, 0)) == -1);
        CHECK(voxel_find(full.data(), 1, voxel_key(1, 0, 0)) == 0 && voxel_find(full.data(), 1, voxel_key(2, 0, 0)) == 1);
    }
    // 2 slots, 1 key: found, and a probe for another key ends from either home slot
    {
        HostTable t;
        std::vector<long long> slot_of;
        CHECK(build({-1, 0, 0}, {0}, 2, &t, &slot_of) && t.view.mask == 1 && voxel_row(t.view, -1, 0, 0) == 0 && voxel_row(t.view, 0, 0, 0) == -1);
        bool homes[2] = {false, false};
        for (int x = 1; x < 40; x++) {
            homes[voxel_hash(voxel_key(x, 0, 0)) & 1] = true;
            CHECK(voxel_find(t.keys.data(), 1, voxel_key(x, 0, 0)) == -1);
        }
        CHECK(homes[0] && homes[1]);
    }
    // a load of exactly one half, 4 keys in 8 slots and 1 024 in 2 048, in ascending and in descending order: every row in a slot of its
    // own, every listed cell found with its row, every other cell of the box absent
    for (int side : {2, 13}) {
        std::vector<int32_t> coord;
        const size_t nv = side == 2 ? 4 : 1024;
        for (int z = 0; z < side && coord.size() < 3 * nv; z++)
            for (int y = 0; y < side && coord.size() < 3 * nv; y++)
                for (int x = 0; x < side && coord.size() < 3 * nv; x++) { coord.push_back(x - 6); coord.push_back(y - 6); coord.push_back(z - 6); }
        for (int descending = 0; descending < 2; descending++) {
            std::vector<int32_t> order(nv);
            for (size_t i = 0; i < nv; i++) order[i] = (int32_t)(descending ? nv - 1 - i : i);
            HostTable t;
            std::vector<long long> slot_of;
            CHECK(build(coord, order, 2, &t, &slot_of) && t.view.mask + 1 == 2 * nv);
            CHECK(std::set<long long>(slot_of.begin(), slot_of.end()).size() == nv);
            size_t at = 0, taken = 0;
            for (unsigned long long k : t.keys) taken += k != VOXEL_KEY_EMPTY;
            CHECK(taken == nv);
            for (int z = -7; z <= side - 6; z++)
                for (int y = -7; y <= side - 6; y++)
                    for (int x = -7; x <= side - 6; x++) {
                        const bool listed = at < nv && coord[3 * at] == x && coord[3 * at + 1] == y && coord[3 * at + 2] == z;
                        CHECK(voxel_row(t.view, x, y, z) == (listed ? (int)at : -1));
                        at += listed;
                    }
            CHECK(at == nv);
        }
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("voxel_table selftest ok\n");
    return 0;
}
