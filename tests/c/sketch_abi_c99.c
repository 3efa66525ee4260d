/*
 * sketch_abi_c99.c -- the HyperLogLog and Count-Min Sketch entry points as cgo
 * sees them: built with gcc -std=c99 -pedantic -Werror
 * (tests/test_sketch_abi.py).  It takes the addresses of the twelve entries
 * through pointers of exactly the declared types and prints the ABI version,
 * the status a null context gets from the ten entries that take one, and what
 * the two pure host functions answer.  No device is touched.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "nkv_merkle.h"

typedef int (*hll_dev_fn)(nkv_ctx *, const void *, const uint64_t *, const uint64_t *, uint64_t, int, void *);
typedef int (*hll_rec_dev_fn)(nkv_ctx *, const void *, uint64_t, const uint64_t *, uint64_t, int, void *);
typedef int (*cms_dev_fn)(nkv_ctx *, const void *, const uint64_t *, const uint64_t *, uint64_t, uint32_t, uint32_t,
                          uint32_t, uint32_t *);
typedef int (*cms_rec_dev_fn)(nkv_ctx *, const void *, uint64_t, const uint64_t *, uint64_t, uint32_t, uint32_t,
                              uint32_t, uint32_t *);
typedef int (*cms_query_dev_fn)(nkv_ctx *, const void *, const uint64_t *, const uint64_t *, uint64_t, uint32_t,
                                uint32_t, uint32_t, const uint32_t *, uint32_t *);
typedef int (*hll_fn)(nkv_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, uint64_t, int, uint8_t *);
typedef int (*hll_rec_fn)(nkv_ctx *, const uint8_t *, uint64_t, const uint64_t *, uint64_t, int, uint8_t *);
typedef int (*cms_fn)(nkv_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, uint64_t, uint32_t, uint32_t,
                      uint32_t, uint32_t *);
typedef int (*cms_rec_fn)(nkv_ctx *, const uint8_t *, uint64_t, const uint64_t *, uint64_t, uint32_t, uint32_t,
                          uint32_t, uint32_t *);
typedef int (*cms_query_fn)(nkv_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, uint64_t, uint32_t,
                            uint32_t, uint32_t, const uint32_t *, uint32_t *);
typedef int (*params_fn)(double, double, uint32_t *, uint32_t *);
typedef int (*estimate_fn)(const uint8_t *, int, int, double *);

int main(void) {
    hll_dev_fn hll_dev = nkv_hll_add_dev;
    hll_rec_dev_fn hll_rec_dev = nkv_hll_add_records_dev;
    cms_dev_fn cms_dev = nkv_cms_insert_dev;
    cms_rec_dev_fn cms_rec_dev = nkv_cms_insert_records_dev;
    cms_query_dev_fn cms_query_dev = nkv_cms_query_dev;
    hll_fn hll = nkv_hll_add;
    hll_rec_fn hll_rec = nkv_hll_add_records;
    cms_fn cms = nkv_cms_insert;
    cms_rec_fn cms_rec = nkv_cms_insert_records;
    cms_query_fn cms_query = nkv_cms_query;
    params_fn params = nkv_cms_params;
    estimate_fn estimate = nkv_hll_estimate;
    uint8_t reg[16] = {0};
    uint32_t table[84] = {0}, out[1] = {7}, m = 0, k = 0;
    const uint8_t key[2] = {1, 2};
    const uint64_t off[1] = {0}, len[1] = {2};
    double est = 0.0;
    int i, rc, touched = 0;
    printf("abi %d\n", nkv_abi_version());
    printf("symbols %d\n", hll_dev != NULL && hll_rec_dev != NULL && cms_dev != NULL && cms_rec_dev != NULL &&
                               cms_query_dev != NULL && hll != NULL && hll_rec != NULL && cms != NULL &&
                               cms_rec != NULL && cms_query != NULL && params != NULL && estimate != NULL);
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d %d %d %d %d %d %d %d %d\n", hll_dev(NULL, key, off, len, 1, 4, reg),
           hll_rec_dev(NULL, key, 2, off, 1, 4, reg), cms_dev(NULL, key, off, len, 1, 28, 3, 0, table),
           cms_rec_dev(NULL, key, 2, off, 1, 28, 3, 0, table),
           cms_query_dev(NULL, key, off, len, 1, 28, 3, 0, table, out), hll(NULL, key, off, len, 1, 4, reg),
           hll_rec(NULL, key, 2, len, 1, 4, reg), cms(NULL, key, off, len, 1, 28, 3, 0, table),
           cms_rec(NULL, key, 2, len, 1, 28, 3, 0, table), cms_query(NULL, key, off, len, 1, 28, 3, 0, table, out));
    for (i = 0; i < 16; ++i) touched |= reg[i] != 0;
    for (i = 0; i < 84; ++i) touched |= table[i] != 0;
    printf("untouched %d\n", !touched && out[0] == 7);
    rc = params(0.1, 0.1, &m, &k);
    printf("params %d %lu %lu\n", rc, (unsigned long)m, (unsigned long)k);
    printf("params_refused %d %d %d\n", params(0.0, 0.1, &m, &k), params(0.1, 0.0, &m, &k),
           params(0.1, 1.0, &m, &k));
    reg[3] = 1;
    rc = estimate(reg, 4, NKV_HLL_ESTIMATE_REFERENCE, &est);
    printf("estimate %d %.17g\n", rc, est);
    printf("constants %d %d %d %d\n", NKV_HLL_MIN_PRECISION, NKV_HLL_MAX_PRECISION, NKV_HLL_ESTIMATE_STANDARD,
           NKV_OPT_SKETCH_PATH);
    return 0;
}
