/*
 * lookup_abi_c99.c -- the point-lookup entry points as cgo sees them: built
 * with gcc -std=c99 -pedantic -Werror (tests/test_lookup_abi.py).  It takes the
 * addresses of the two entries through pointers of exactly the declared types,
 * fills an nkv_lookup_table, and prints the ABI version, the constants and the
 * status a null context gets.  No device is touched.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "nkv_merkle.h"

typedef int (*lookup_fn)(nkv_ctx *, const nkv_lookup_table *, int, const void *, const uint64_t *, const uint64_t *,
                         uint64_t, uint64_t *, uint8_t *, uint8_t *, uint32_t *);
typedef int (*values_fn)(nkv_ctx *, const nkv_lookup_table *, int, const uint64_t *, const uint8_t *, uint64_t,
                         void *, uint64_t, uint64_t *, uint64_t *);

int main(void) {
    lookup_fn lookup = nkv_lookup_dev;
    values_fn values = nkv_lookup_values_dev;
    nkv_lookup_table tab;
    uint64_t out_len = 7;
    tab.stream = NULL;
    tab.stream_len = 0;
    tab.rec_off = NULL;
    tab.n = 1;
    tab.bits = NULL;
    tab.m = 64;
    tab.k = 2;
    tab.seed0 = 1;
    printf("abi %d\n", nkv_abi_version());
    printf("symbols %d\n", lookup != NULL && values != NULL);
    printf("constants %d %d %d %d %d %d %d %d %d\n", NKV_LOOKUP_MAX_TABLES, NKV_STAGE_NOT_SEARCHED, NKV_STAGE_FILTER,
           NKV_STAGE_SUMMARY, NKV_STAGE_INDEX, NKV_STAGE_FOUND, NKV_GET_ABSENT, NKV_GET_LIVE, NKV_GET_TOMBSTONE);
    printf("struct %u %u %u\n", (unsigned)sizeof(nkv_lookup_table), (unsigned)offsetof(nkv_lookup_table, bits),
           (unsigned)offsetof(nkv_lookup_table, seed0));
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d\n", lookup(NULL, &tab, 1, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL),
           values(NULL, &tab, 1, NULL, NULL, 0, NULL, 0, NULL, &out_len));
    return 0;
}
