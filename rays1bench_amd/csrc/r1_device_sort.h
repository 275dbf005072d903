// r1_device_sort.h — the block size, the scratch sizes and the arguments of the device's one prefix sum and one radix sort
// (r1_device_sort.hip; the functions that launch them: r1_internal.h).  Plain C++: the host lays the scratch out with it.
#ifndef R1_DEVICE_SORT_H
#define R1_DEVICE_SORT_H

#include <stddef.h>
#include <stdint.h>

#define R1_SORT_BLOCK 256 // lanes per workgroup = items per workgroup, in every kernel of the three files: the tests count with it

// workgroups of n items
inline unsigned r1_blocks(size_t n) { return (unsigned)((n + R1_SORT_BLOCK - 1) / R1_SORT_BLOCK); }

// words of block sums a prefix sum over n items needs, all levels
inline size_t r1_scan_sums_words(size_t n)
{
    size_t words = 0;
    while (n > R1_SORT_BLOCK)
        n = r1_blocks(n), words += n;
    return words;
}

// words of digit counts a sort of `lists` lists of up to n_max items needs; its prefix sum takes r1_scan_sums_words() of as many items
inline size_t r1_radix_hist_words(size_t n_max, size_t lists) { return lists * 256 * r1_blocks(n_max); }

// What r1_radix_sort_enqueue sorts, device memory: `lists` lists laid end to end with stride n_max, each by its own keys, stably; the values
// travel with the keys.  Two buffers of each, taken in turn by the passes: the input is in [0].
struct R1RadixArgs
{
    uint32_t *key[2], *val[2]; // [lists * n_max] each
    uint32_t *hist;            // [r1_radix_hist_words(n_max, lists)] the per-block digit counts, then their exclusive prefix sum (in place)
    uint32_t *sums;            // [r1_scan_sums_words(of as many)] that prefix sum's block sums
    uint32_t n_max;            // items per list: what the launches are sized for, and the bound that guards every store
    uint32_t lists;
    const uint32_t *n_dev;     // null: every list holds n_max items; or the count in device memory, taken as n_max where it is larger
};

#endif
