/*
 * locate_abi_c99.c -- the index-lookup entry points as cgo sees them: built
 * with gcc -std=c99 -pedantic -Werror (tests/test_locate_abi.py).  It takes the
 * addresses of the two entries through pointers of exactly the declared types,
 * fills an nkv_index_table, and prints the ABI version, the constants and the
 * status a null context gets.  No device is touched.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "nkv_merkle.h"

typedef int (*open_fn)(nkv_ctx *, const void *, uint64_t, const void *, uint64_t, uint64_t *, uint64_t, uint64_t *,
                       uint64_t *, uint32_t *);
typedef int (*locate_fn)(nkv_ctx *, const nkv_index_table *, int, uint32_t, const void *, const uint64_t *,
                         const uint64_t *, uint64_t, int, uint64_t *, int64_t *, uint8_t *, uint8_t *, uint32_t *);

int main(void) {
    open_fn open = nkv_index_open_dev;
    locate_fn locate = nkv_locate_dev;
    nkv_index_table tab;
    uint64_t n = 7, s = 7;
    uint32_t verdict = 7;
    uint8_t image[32] = {0};
    tab.index = NULL;
    tab.index_len = 0;
    tab.ent_off = NULL;
    tab.n = 1;
    tab.bits = NULL;
    tab.m = 64;
    tab.k = 2;
    tab.seed0 = 1;
    printf("abi %d\n", nkv_abi_version());
    printf("symbols %d\n", open != NULL && locate != NULL);
    printf("constants %d %d %d %d %d %d %d %d %d\n", NKV_INDEX_BAD_HEADER, NKV_INDEX_BAD_SUMMARY_CHAIN,
           NKV_INDEX_BAD_INDEX_CHAIN, NKV_INDEX_BAD_LINK, NKV_INDEX_BAD_ORDER, NKV_INDEX_BAD_RANGE, NKV_GET_LOCATED,
           NKV_OPT_INDEX_OPEN_PATH, NKV_OPT_INDEX_OPEN_CHUNK);
    printf("struct %u %u %u %u %u\n", (unsigned)sizeof(nkv_index_table), (unsigned)offsetof(nkv_index_table, index_len),
           (unsigned)offsetof(nkv_index_table, ent_off), (unsigned)offsetof(nkv_index_table, bits),
           (unsigned)offsetof(nkv_index_table, seed0));
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d\n", open(NULL, image, 32, image, 32, NULL, 0, &n, &s, &verdict),
           locate(NULL, &tab, 1, 0, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL, NULL));
    return 0;
}
