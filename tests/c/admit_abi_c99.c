/*
 * admit_abi_c99.c -- the admission entry point as cgo sees it: built with gcc
 * -std=c99 -pedantic -Werror (tests/test_admit_abi.py).  It takes the address
 * of nkv_admit_dev through a pointer of exactly the declared type, fills an
 * nkv_requests field by field, and prints the ABI version, the constants, the
 * struct's size and the status a null context and a null request get.  No
 * device is touched.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "nkv_merkle.h"

typedef int (*admit_fn)(nkv_ctx *, const nkv_requests *, const void *, uint64_t, int64_t, int64_t, uint8_t *, void *,
                        int64_t *, uint64_t *, uint8_t *, uint32_t *);

int main(void) {
    admit_fn admit = nkv_admit_dev;
    nkv_requests r;
    uint8_t verdict[1];
    r.users = NULL, r.users_len = 0, r.uoff = NULL, r.ulen = NULL;
    r.keys = NULL, r.keys_len = 0, r.koff = NULL, r.klen = NULL;
    r.ts = NULL, r.ts_all = 0;
    r.buckets = NULL, r.boff = NULL, r.bstatus = NULL;
    r.n = 0;
    verdict[0] = 0;
    printf("abi %d\n", nkv_abi_version());
    printf("symbols %d\n", admit != NULL);
    printf("constants %d %d %d %d %d %d %d\n", NKV_ADMIT_ILLEGAL, NKV_ADMIT_ALLOWED, NKV_ADMIT_THROTTLED,
           NKV_ADMIT_BAD_SPAN, NKV_ADMIT_BAD_KEY, NKV_ADMIT_BAD_TIME, NKV_ADMIT_BAD_BUCKET);
    printf("sizeof %lu\n", (unsigned long)sizeof(nkv_requests));
    /* a null context is refused before anything else happens */
    printf("null_ctx %d %d\n", admit(NULL, &r, "$", 1, 100, 1, verdict, NULL, NULL, NULL, NULL, NULL),
           admit(NULL, NULL, "$", 1, 100, 1, verdict, NULL, NULL, NULL, NULL, NULL));
    return 0;
}
