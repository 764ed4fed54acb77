// The index arithmetic of libprosstt_amd_ranks.so's sort and fold kernels (ranks.hip), said once and free of HIP: which
// position a thread takes, which lanes of its wave share its digit, where an entry is scattered to, and how the runs' starts
// and ends are carried along a segment.  It compiles for the host too, so that a plain C++ program can walk the very same
// arithmetic over whole segments under a sanitizer before a kernel ever runs: every scatter offset and every LDS slot below
// is a function of (tile, item, thread, digit, ballots) alone.
// Internal: included by ranks/ranks.hip, and not installed under include/.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RANKS_HD __host__ __device__ __forceinline__
#else
#define RANKS_HD inline
#endif

namespace ranks_index {

constexpr int kBlock = 256;                 // threads of every kernel
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kDigits = 256;                // a radix pass takes 8 key bits: thread d of the block owns digit d
constexpr int kDigitBits = 8;
constexpr int kItems = 4;                   // entries per thread and tile of the sort
constexpr int kSortTile = kBlock * kItems;  // = PROSSTT_AMD_RANKS_SORT_TILE
constexpr int kSlots = kItems * kWaves;     // (item, wave) pairs of a tile, in position order
constexpr int32_t kNoStart = -1;            // below every position and every count: neutral for max
constexpr int32_t kNoEnd = INT32_MAX;       // above every position and every count: neutral for min

// ------------------------------------------------------------------------------------------------------------- sort

// A tile is striped: item i of thread t is position tile * kSortTile + i * kBlock + t, so position order within a tile is
// (item, wave, lane) ascending.
RANKS_HD int64_t sort_position(int64_t tile, int item, int tid)
{
    return tile * kSortTile + (int64_t)item * kBlock + tid;
}

RANKS_HD uint32_t digit_of(uint32_t key, int shift) { return (key >> shift) & (uint32_t)(kDigits - 1); }

RANKS_HD uint64_t lanes_below(int lane) { return (uint64_t(1) << lane) - 1; }
RANKS_HD uint64_t lanes_above(int lane) { return lane == kWave - 1 ? 0 : ~uint64_t(0) << (lane + 1); }
RANKS_HD int bits_set(uint64_t m) { return __builtin_popcountll(m); }

// The lanes of the wave that hold an entry (valid) with this lane's digit.  bit_ballot[b]: the lanes whose digit has bit b.
RANKS_HD uint64_t peers(uint32_t digit, const uint64_t (&bit_ballot)[kDigitBits], uint64_t valid)
{
    uint64_t m = valid;
    for (int b = 0; b < kDigitBits; ++b) m &= ((digit >> b) & 1u) ? bit_ballot[b] : ~bit_ballot[b];
    return m;
}

// The first of its peers writes their number down for the whole wave.
RANKS_HD bool leads(uint64_t peer_lanes, int lane) { return (peer_lanes & lanes_below(lane)) == 0; }

// counts / offsets [kSlots][kDigits]: slot (item, wave) of a digit.
RANKS_HD int count_slot(int item, int wave, uint32_t digit) { return (item * kWaves + wave) * kDigits + (int)digit; }

// Thread `digit` after a tile's counts are in: offsets[slot] = where the first entry of that (item, wave) with this digit
// goes, continuing from base[digit]; base moves on by the tile's total, and the counts are zeroed for the next tile.
RANKS_HD void tile_offsets(uint8_t* counts, uint32_t* offsets, uint32_t* base, int digit)
{
    uint32_t run = base[digit];
    for (int s = 0; s < kSlots; ++s) {
        const int at = s * kDigits + digit;
        offsets[at] = run;
        run += counts[at];
        counts[at] = 0;
    }
    base[digit] = run;
}

// Where an entry goes: behind its peers in lower lanes.  Stable: position order is (item, wave, lane).
RANKS_HD uint32_t destination(const uint32_t* offsets, int item, int wave, uint32_t digit, uint64_t peer_lanes, int lane)
{
    return offsets[count_slot(item, wave, digit)] + (uint32_t)bits_set(peer_lanes & lanes_below(lane));
}

// ------------------------------------------------------------------------------------------------------------- fold

// A fold tile is kBlock consecutive positions, thread t at tile * kBlock + t.
RANKS_HD int64_t fold_position(int64_t tile, int tid) { return tile * kBlock + tid; }

// The segmented scans within a wave are read off ballots: `marks` are the lanes at a run's first (up) or last (down)
// position, and a lane's run starts at the nearest marked lane at or below it, and ends at the nearest at or above it (-1: not
// in this wave).
RANKS_HD int nearest_at_or_below(uint64_t marks, int lane)
{
    const uint64_t m = marks & (lanes_below(lane) | (uint64_t(1) << lane));
    return m ? kWave - 1 - __builtin_clzll(m) : -1;
}
RANKS_HD int nearest_at_or_above(uint64_t marks, int lane)
{
    const uint64_t m = marks & ~lanes_below(lane);
    return m ? __builtin_ctzll(m) : -1;
}
// Up: the members of C below the run's first position, within the wave.  Down: those above its last position.
RANKS_HD int32_t start_count_local(uint64_t heads, uint64_t members, int lane)
{
    const int at = nearest_at_or_below(heads, lane);
    return at < 0 ? kNoStart : bits_set(members & lanes_below(at));
}
RANKS_HD int32_t end_count_local(uint64_t tails, uint64_t members, int lane)
{
    const int at = nearest_at_or_above(tails, lane);
    return at < 0 ? kNoStart : bits_set(members & lanes_above(at));
}
// Down: the run's end (one past its last position) as far as the wave knows it.
RANKS_HD int32_t end_local(uint64_t tails, int64_t tile, int wave, int lane)
{
    const int at = nearest_at_or_above(tails, lane);
    return at < 0 ? kNoEnd : (int32_t)(fold_position(tile, wave * kWave + at) + 1);
}

// Those counts are local to the wave (the members of C in lower lanes, or in higher lanes): every lane of a wave lacks the
// same addend, so the maximum commutes with adding it.  What reaches a wave from outside -- the carry
// of the tiles already walked and the other waves of this tile on that side -- comes through three words per wave in LDS:
// wave_total (its members of C), and the local values above at its last (up) or first (down) lane.  With wave = kWaves (up) or
// wave = -1 (down) the same functions give the carries for the next tile.
RANKS_HD int32_t count_before(const int32_t* wave_total, int wave)
{
    int32_t c = 0;
    for (int w = 0; w < wave; ++w) c += wave_total[w];
    return c;
}
RANKS_HD int32_t count_after(const int32_t* wave_total, int wave)
{
    int32_t c = 0;
    for (int w = wave + 1; w < kWaves; ++w) c += wave_total[w];
    return c;
}
RANKS_HD int32_t lifted(int32_t local, int32_t addend) { return local == kNoStart ? kNoStart : local + addend; }

// Up.  P[start of the run] as far as the tiles before (carry; `counted` members of C in them) and the waves below know it:
// wave_start[w] is wave w's largest local count at a run's first position, or kNoStart.
RANKS_HD int32_t start_count_below(const int32_t* wave_total, const int32_t* wave_start, int wave, int32_t counted,
                                   int32_t carry)
{
    int32_t lift = counted;
    for (int w = 0; w < wave; ++w) {
        const int32_t here = lifted(wave_start[w], lift);
        carry = here > carry ? here : carry;
        lift += wave_total[w];
    }
    return carry;
}

// Down.  The end of the run (a position) as far as the tiles after and the waves above know it.
RANKS_HD int32_t end_above(const int32_t* wave_end, int wave, int32_t carry)
{
    for (int w = wave + 1; w < kWaves; ++w) carry = wave_end[w] < carry ? wave_end[w] : carry;
    return carry;
}
// Down.  P[end of the run] likewise: wave_most[w] is wave w's largest local count of members ABOVE a run's last position (its
// lowest such position: the nearest one for everything below), or kNoStart; `after` members of C lie in the tiles after, and
// P[p + 1] = members_total - (the members above p).
RANKS_HD int32_t end_count_above(const int32_t* wave_total, const int32_t* wave_most, int wave, int32_t after,
                                 int32_t members_total, int32_t carry)
{
    int32_t lift = after;
    for (int w = kWaves - 1; w > wave; --w) {
        if (wave_most[w] != kNoStart) carry = members_total - (lift + wave_most[w]);
        lift += wave_total[w];
    }
    return carry;
}

// t^3 - t of a run of t equal values (t <= 2^20: below 2^60).
RANKS_HD uint64_t tie_term(int64_t t) { return (uint64_t)(t * t * t - t); }

}  // namespace ranks_index
