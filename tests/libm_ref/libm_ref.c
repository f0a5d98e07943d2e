/* libm_ref.c — TEST INFRASTRUCTURE: this machine's libm and IEEE fp32 arithmetic, one function per call, over a range of bit
 * patterns or over arrays, and the comparison of such results with a buffer of device results (tests/test_device_math.py).
 *
 * Build: gcc -O1 -fno-builtin -shared -fPIC -o libm_ref.so libm_ref.c -lm -lpthread
 * (-fno-builtin: every call below goes to libm.so.6, the libm the compiled reference calls; nothing is folded).
 *
 * The comparison is done here, not in Python: a sweep returns a count and the first <= 64 mismatches, never an array.
 * Two results are equal if their bits are equal, or if both are NaN. Work is split over at most 8 threads created here
 * (a fixed bound, never the machine's CPU count). */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <string.h>

enum { FN_SINF = 0, FN_COSF, FN_SINF_2PI, FN_COSF_2PI, FN_LOGF, FN_EXPF, FN_LOG2F, FN_POWF, FN_DIV, FN_SQRT, FN_BREV, FN_COUNT,
       FN_COPY = 100 /* the reference result is operand a itself: feeds the comparison a buffer of known values */ };
enum { MAX_THREADS = 8, MAX_REPORTED = 64, MIN_PER_THREAD = 1 << 14 };

typedef struct { uint32_t a, b, device, libm; } LibmRefMismatch;   /* operand bits (b: second operand / exponent), both results */

static float f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t u32(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* one function per libm call */
static uint32_t ref_sinf(uint32_t a) { return u32(sinf(f32(a))); }
static uint32_t ref_cosf(uint32_t a) { return u32(cosf(f32(a))); }
static uint32_t ref_logf(uint32_t a) { return u32(logf(f32(a))); }
static uint32_t ref_expf(uint32_t a) { return u32(expf(f32(a))); }
static uint32_t ref_log2f(uint32_t a) { return u32(log2f(f32(a))); }
static uint32_t ref_powf(uint32_t a, uint32_t b) { return u32(powf(f32(a), f32(b))); }
/* IEEE fp32 divide and square root of the CPU, through volatile operands so that nothing is folded or widened */
static uint32_t ref_div(uint32_t a, uint32_t b) { volatile float x = f32(a), y = f32(b); volatile float q = x / y; return u32(q); }
static uint32_t ref_sqrtf(uint32_t a) { volatile float x = f32(a); volatile float r = sqrtf(x); return u32(r); }
/* the host form of reverseBits32 (csrc/ymath.hpp; reference math.hpp:102-109) */
static uint32_t ref_brev(uint32_t n) {
  n = (n << 16) | (n >> 16);
  n = ((n & 0x00ff00ffu) << 8) | ((n & 0xff00ff00u) >> 8);
  n = ((n & 0x0f0f0f0fu) << 4) | ((n & 0xf0f0f0f0u) >> 4);
  n = ((n & 0x33333333u) << 2) | ((n & 0xccccccccu) >> 2);
  n = ((n & 0x55555555u) << 1) | ((n & 0xaaaaaaaau) >> 1);
  return n;
}

static int known(int fn) { return (fn >= 0 && fn < FN_COUNT) || fn == FN_COPY; }
static uint32_t eval(int fn, uint32_t a, uint32_t b) {
  switch (fn) {
    case FN_SINF: case FN_SINF_2PI: return ref_sinf(a);
    case FN_COSF: case FN_COSF_2PI: return ref_cosf(a);
    case FN_LOGF: return ref_logf(a);
    case FN_EXPF: return ref_expf(a);
    case FN_LOG2F: return ref_log2f(a);
    case FN_POWF: return ref_powf(a, b);
    case FN_DIV: return ref_div(a, b);
    case FN_SQRT: return ref_sqrtf(a);
    case FN_BREV: return ref_brev(a);
    default: return a;   /* FN_COPY */
  }
}

static int is_nan(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }
/* THE equality of every comparison in this file */
static int same(uint32_t x, uint32_t y) { return x == y || (is_nan(x) && is_nan(y)); }

typedef struct {
  int fn;
  uint32_t first_bits, y_bits;
  const uint32_t *a, *b, *device;   /* a == NULL: the range form */
  uint32_t* ref_out;                /* != NULL: also store the reference results */
  uint64_t lo, hi;
  uint64_t mismatches;
  LibmRefMismatch first[MAX_REPORTED];
} Job;

static void* worker(void* p) {
  Job* j = (Job*)p;
  for (uint64_t i = j->lo; i < j->hi; i++) {
    const uint32_t a = j->a ? j->a[i] : j->first_bits + (uint32_t)i;
    const uint32_t b = j->b ? j->b[i] : j->y_bits;
    const uint32_t r = eval(j->fn, a, b);
    if (j->ref_out) j->ref_out[i] = r;
    if (j->device && !same(j->device[i], r)) {
      if (j->mismatches < MAX_REPORTED) {
        LibmRefMismatch* m = &j->first[j->mismatches];
        m->a = a; m->b = b; m->device = j->device[i]; m->libm = r;
      }
      j->mismatches++;
    }
  }
  return 0;
}

/* Evaluates fn over n inputs — a[i] (and b[i]), or with a == NULL the bit patterns first_bits + i (second operand y_bits) —
 * and compares with device[i]. Returns the number of mismatches, or UINT64_MAX for a bad argument; first_out (room for 64)
 * receives the first min(count, 64) mismatches in input order. ref_out, if not NULL, receives the n reference results. */
uint64_t libm_ref_check(int fn, uint32_t first_bits, uint64_t n, uint32_t y_bits, const uint32_t* a, const uint32_t* b,
                        const uint32_t* device, LibmRefMismatch* first_out, uint32_t* ref_out) {
  static Job jobs[MAX_THREADS];
  static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
  if (!known(fn) || n == 0 || (!device && !ref_out) || (device && !first_out)) return UINT64_MAX;
  if (!a && (uint64_t)first_bits + n > (1ull << 32)) return UINT64_MAX;
  pthread_mutex_lock(&mu);
  int nt = (int)(n / MIN_PER_THREAD);
  if (nt < 1) nt = 1;
  if (nt > MAX_THREADS) nt = MAX_THREADS;
  pthread_t th[MAX_THREADS];
  int started[MAX_THREADS];
  for (int t = 0; t < nt; t++) {
    Job* j = &jobs[t];
    j->fn = fn; j->first_bits = first_bits; j->y_bits = y_bits; j->a = a; j->b = b; j->device = device; j->ref_out = ref_out;
    j->lo = n * (uint64_t)t / (uint64_t)nt; j->hi = n * (uint64_t)(t + 1) / (uint64_t)nt;
    j->mismatches = 0;
    started[t] = t > 0 && pthread_create(&th[t], 0, worker, j) == 0;
  }
  worker(&jobs[0]);
  for (int t = 1; t < nt; t++) {
    if (started[t]) pthread_join(th[t], 0);
    else worker(&jobs[t]);          /* no thread to be had: do the slice here */
  }
  uint64_t total = 0;
  for (int t = 0; t < nt; t++) {
    for (uint64_t k = 0; k < jobs[t].mismatches && k < MAX_REPORTED; k++)
      if (total + k < MAX_REPORTED) first_out[total + k] = jobs[t].first[k];
    total += jobs[t].mismatches;
  }
  pthread_mutex_unlock(&mu);
  return total;
}

/* the number of threads libm_ref_check uses for n inputs (for the tests' report) */
int libm_ref_threads(uint64_t n) {
  uint64_t nt = n / MIN_PER_THREAD;
  return nt < 1 ? 1 : (nt > MAX_THREADS ? MAX_THREADS : (int)nt);
}
