/*
 * sort_abi_c99.c -- the memtable-flush entry points as cgo sees them: built
 * with gcc -std=c99 -pedantic -Werror (tests/test_sort_abi.py).  It takes the
 * addresses of the two entries through pointers of exactly the declared types
 * and prints the ABI version and the status a null context gets.  No device is
 * touched.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "nkv_merkle.h"

typedef int (*sort_dev_fn)(nkv_ctx *, const void *, uint64_t, const uint64_t *, uint64_t, void *, uint64_t, uint64_t *,
                           uint64_t *, uint64_t *, uint64_t *);
typedef int (*sort_fn)(nkv_ctx *, const uint8_t *, uint64_t, const uint64_t *, uint64_t, uint8_t *, uint64_t,
                       uint64_t *, uint64_t *, uint64_t *);

int main(void) {
    sort_dev_fn sort_dev = nkv_sort_records_dev;
    sort_fn sort = nkv_sort_records;
    uint64_t n_out = 7, out_len = 7;
    printf("abi %d\n", nkv_abi_version());
    printf("symbols %d\n", sort_dev != NULL && sort != NULL);
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d\n", sort_dev(NULL, NULL, 0, NULL, 0, NULL, 0, NULL, NULL, &n_out, &out_len),
           sort(NULL, NULL, 0, NULL, 0, NULL, 0, NULL, &n_out, &out_len));
    printf("untouched %d\n", n_out == 7 && out_len == 7);
    return 0;
}
