// The voxel hash table of the NDT map (K30, K31), the TSDF map (K71, K72, K75) and the ray cast's skip blocks (K73, K74), stated once for
// the device kernels (ndt_kernels.hip, tsdf_kernels.hip), the drivers (ndt_api.hip, tsdf_api.hip) and the CPU self-test
// (tests/voxel_table_selftest.cpp, which includes this header alone, without HIP).
//   Layout   open addressing, linear probing, a power of two of slots.  keys[slot] is the packed coordinate of the voxel stored there, or
//            VOXEL_KEY_EMPTY; vals[slot] its row in the caller's list (a key-only table has no vals).  At most half the slots are ever taken
//            (1 / 27 of them in K74's table), so a probe always ends at a free slot.
//   Key      (cx - cmin_x) | (cy - cmin_y) << 20 | (cz - cmin_z) << 40, every term in [0, ext) with ext <= 2^20: 60 bits, so no key is
//            VOXEL_KEY_EMPTY.  A driver refuses a list that spans more than 2^20 voxels along an axis before a key is formed.
//   Hash     splitmix64's finaliser, masked to the slots.
//   Claim    a lane claims the first free slot from its hash by a 64-bit compare-and-swap; a key met again is left where it is.  Keys that
//            are unique find the same row whatever order the lanes arrived in.  On the host the same loop runs with a plain compare-and-set.
#pragma once

#if defined(__HIPCC__)
#define MISLAM_VOXEL_HD __host__ __device__ __forceinline__
#else
#define MISLAM_VOXEL_HD inline
#endif

namespace mislam {

constexpr unsigned long long VOXEL_KEY_EMPTY = 0xffffffffffffffffull;   // a free slot
constexpr int VOXEL_KEY_BITS = 20;                                       // of the key per axis
constexpr long long VOXEL_MAX_EXTENT = 1ll << VOXEL_KEY_BITS;            // voxels per axis between the lowest and the highest listed one

struct VoxelTableView {
    const unsigned long long* keys;  // mask + 1 slots
    const int* vals;                 // null: a key-only table
    unsigned long long mask;         // slots - 1
    int cmin[3], ext[3];             // the frame: a key is formed for (cx, cy, cz) in [cmin, cmin + ext) alone
};

// the key of a coordinate relative to cmin, each in [0, 2^20), and back
MISLAM_VOXEL_HD unsigned long long voxel_key(int rx, int ry, int rz)
{
    return (unsigned long long)rx | (unsigned long long)ry << VOXEL_KEY_BITS | (unsigned long long)rz << 2 * VOXEL_KEY_BITS;
}
MISLAM_VOXEL_HD int voxel_key_axis(unsigned long long key, int axis) { return (int)(key >> axis * VOXEL_KEY_BITS & (unsigned long long)(VOXEL_MAX_EXTENT - 1)); }

// false: (cx, cy, cz) is outside the frame and no key is formed (the differences in 64 bits: coordinates near +-2^30 stay right)
MISLAM_VOXEL_HD bool voxel_key_in_frame(const VoxelTableView& t, int cx, int cy, int cz, unsigned long long* key)
{
    const long long rx = (long long)cx - t.cmin[0], ry = (long long)cy - t.cmin[1], rz = (long long)cz - t.cmin[2];
    if (rx < 0 || rx >= t.ext[0] || ry < 0 || ry >= t.ext[1] || rz < 0 || rz >= t.ext[2]) return false;
    *key = voxel_key((int)rx, (int)ry, (int)rz);
    return true;
}

MISLAM_VOXEL_HD unsigned long long voxel_hash(unsigned long long key)      // splitmix64's finaliser
{
    key ^= key >> 30; key *= 0xbf58476d1ce4e5b9ull;
    key ^= key >> 27; key *= 0x94d049bb133111ebull;
    return key ^ (key >> 31);
}

// the slot that holds `key`, or -1
MISLAM_VOXEL_HD long long voxel_find(const unsigned long long* keys, unsigned long long mask, unsigned long long key)
{
    unsigned long long slot = voxel_hash(key) & mask;
    for (unsigned long long probe = 0; probe <= mask; probe++) {
        const unsigned long long k = keys[slot];
        if (k == key) return (long long)slot;
        if (k == VOXEL_KEY_EMPTY) return -1;
        slot = (slot + 1) & mask;
    }
    return -1;
}
// the row of voxel (cx, cy, cz), or -1: outside the frame or not in the table
MISLAM_VOXEL_HD int voxel_row(const VoxelTableView& t, int cx, int cy, int cz)
{
    unsigned long long key;
    if (!voxel_key_in_frame(t, cx, cy, cz, &key)) return -1;
    const long long slot = voxel_find(t.keys, t.mask, key);
    return slot < 0 ? -1 : t.vals[slot];
}
MISLAM_VOXEL_HD bool voxel_present(const VoxelTableView& t, int cx, int cy, int cz)
{
    unsigned long long key;
    return voxel_key_in_frame(t, cx, cy, cz, &key) && voxel_find(t.keys, t.mask, key) >= 0;
}

// the slot `key` has after the call (-1: no slot was free, which a table that holds its keys never sees); *fresh (may be null): the call
// put it there.  A caller with values writes vals[slot] either way.
MISLAM_VOXEL_HD long long voxel_claim(unsigned long long* keys, unsigned long long mask, unsigned long long key, bool* fresh = nullptr)
{
    if (fresh) *fresh = false;
    unsigned long long slot = voxel_hash(key) & mask;
    for (unsigned long long probe = 0; probe <= mask; probe++) {
#if defined(__HIP_DEVICE_COMPILE__)
        const unsigned long long old = atomicCAS(&keys[slot], VOXEL_KEY_EMPTY, key);
#else
        const unsigned long long old = keys[slot];
        if (old == VOXEL_KEY_EMPTY) keys[slot] = key;
#endif
        if (old == VOXEL_KEY_EMPTY && fresh) *fresh = true;
        if (old == VOXEL_KEY_EMPTY || old == key) return (long long)slot;
        slot = (slot + 1) & mask;
    }
    return -1;
}

// ---- the host's side
// slots for n keys at `per` slots per key: the least power of two >= per n, 2 at least
inline unsigned long long voxel_table_slots(unsigned long long n, unsigned long long per)
{
    unsigned long long slots = 2;
    while (slots < per * n) slots <<= 1;
    return slots;
}
// does a table of mask + 1 slots hold n keys at `per` slots per key?  (what every launch wrapper asks before its kernel probes)
inline bool voxel_table_holds(unsigned long long mask, unsigned long long n, unsigned long long per) { return (mask & (mask + 1)) == 0 && mask + 1 >= per * n; }
inline long long voxel_extent(const int cmin[3], const int cmax[3], int axis) { return (long long)cmax[axis] - (long long)cmin[axis] + 1; }
// the frame of the coordinates in [cmin, cmax] -> -1, or the first axis whose extent is outside [1, 2^20] (the axes behind it are not set)
inline int voxel_table_frame(VoxelTableView* t, const int cmin[3], const int cmax[3])
{
    for (int a = 0; a < 3; a++) {
        const long long extent = voxel_extent(cmin, cmax, a);
        if (extent < 1 || extent > VOXEL_MAX_EXTENT) return a;
        t->cmin[a] = cmin[a]; t->ext[a] = (int)extent;
    }
    return -1;
}
inline void voxel_table_bind(VoxelTableView* t, const unsigned long long* keys, const int* vals, unsigned long long slots) { t->keys = keys; t->vals = vals; t->mask = slots - 1; }
#if defined(__HIPCC__)
// every slot free
inline hipError_t voxel_table_clear(unsigned long long* keys, unsigned long long slots, hipStream_t s) { return hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * slots, s); }
#endif

}  // namespace mislam
