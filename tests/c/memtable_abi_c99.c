/*
 * memtable_abi_c99.c -- the live memtable's entry points as cgo sees them: built
 * with gcc -std=c99 -pedantic -Werror (tests/test_memtable_abi.py).  It takes
 * the addresses of the four entries through pointers of exactly the declared
 * types and prints the ABI version, the constants, nkv_memtable_index_bytes of
 * a few slot counts and the status a null context gets.  No device is touched.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "nkv_merkle.h"

typedef uint64_t (*bytes_fn)(uint64_t);
typedef int (*clear_fn)(nkv_ctx *, void *, uint64_t, uint64_t *);
typedef int (*add_fn)(nkv_ctx *, const void *, uint64_t, const uint64_t *, uint64_t, uint64_t, void *, uint64_t, int,
                      uint64_t, uint64_t, uint64_t *, uint8_t *, uint32_t *);
typedef int (*find_fn)(nkv_ctx *, const void *, uint64_t, const uint64_t *, uint64_t, const void *, uint64_t,
                       const void *, const uint64_t *, const uint64_t *, uint64_t, uint32_t, int, uint64_t *,
                       uint8_t *, uint32_t *);

int main(void) {
    bytes_fn nbytes = nkv_memtable_index_bytes;
    clear_fn clear = nkv_memtable_clear_dev;
    add_fn add = nkv_memtable_add_dev;
    find_fn find = nkv_memtable_find_dev;
    uint64_t state[NKV_MEMTABLE_STATE_WORDS];
    uint64_t index[2];
    state[0] = index[0] = 0;
    printf("abi %d\n", nkv_abi_version());
    printf("symbols %d\n", nbytes != NULL && clear != NULL && add != NULL && find != NULL);
    printf("constants %d %d %d\n", NKV_FLUSH_BY_CAPACITY, NKV_FLUSH_BY_THRESHOLD, NKV_MEMTABLE_STATE_WORDS);
    printf("index_bytes %lu %lu %lu %lu %lu %lu\n", (unsigned long)nbytes(0), (unsigned long)nbytes(3),
           (unsigned long)nbytes((uint64_t)1 << 33), (unsigned long)nbytes(1), (unsigned long)nbytes(2),
           (unsigned long)nbytes((uint64_t)1 << 32));
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d %d\n", clear(NULL, index, 2, state),
           add(NULL, NULL, 0, NULL, 0, 0, index, 2, 3, 10, 2000, state, NULL, NULL),
           find(NULL, NULL, 0, NULL, 0, index, 2, NULL, NULL, NULL, 0, 0, 0, NULL, NULL, NULL));
    return 0;
}
