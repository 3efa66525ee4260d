/*
 * encode_abi_c99.c -- the record-encode entry points as cgo sees them: built
 * with gcc -std=c99 -pedantic -Werror (tests/test_encode_abi.py).  It takes the
 * addresses of the two entries through pointers of exactly the declared types
 * and prints the ABI version, the status a null context gets, and the size and
 * field offsets of nkv_puts as this compiler lays it out.  No device is
 * touched.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "nkv_merkle.h"

typedef int (*encode_dev_fn)(nkv_ctx *, const nkv_puts *, void *, uint64_t, uint64_t *, uint32_t *, uint64_t *);
typedef int (*encode_fn)(nkv_ctx *, const nkv_puts *, uint8_t *, uint64_t, uint64_t *, uint32_t *, uint64_t *);

int main(void) {
    encode_dev_fn encode_dev = nkv_encode_records_dev;
    encode_fn encode = nkv_encode_records;
    nkv_puts puts = {0};
    uint64_t out_len = 7;
    printf("abi %d\n", nkv_abi_version());
    printf("symbols %d\n", encode_dev != NULL && encode != NULL);
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d\n", encode_dev(NULL, &puts, NULL, 0, NULL, NULL, &out_len),
           encode(NULL, &puts, NULL, 0, NULL, NULL, &out_len));
    printf("untouched %d\n", out_len == 7);
    printf("sizeof %lu\n", (unsigned long)sizeof(nkv_puts));
    printf("offsets %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)offsetof(nkv_puts, keys),
           (unsigned long)offsetof(nkv_puts, keys_len), (unsigned long)offsetof(nkv_puts, koff),
           (unsigned long)offsetof(nkv_puts, klen), (unsigned long)offsetof(nkv_puts, vals),
           (unsigned long)offsetof(nkv_puts, vals_len), (unsigned long)offsetof(nkv_puts, voff),
           (unsigned long)offsetof(nkv_puts, vlen), (unsigned long)offsetof(nkv_puts, ts),
           (unsigned long)offsetof(nkv_puts, ts_all), (unsigned long)offsetof(nkv_puts, status),
           (unsigned long)offsetof(nkv_puts, type), (unsigned long)offsetof(nkv_puts, n));
    return 0;
}
