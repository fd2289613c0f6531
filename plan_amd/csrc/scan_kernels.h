// Parameter blocks of the fused scan kernels (scan_kernels.hip), filled by scan_plan.hip, and their launches. Which kernel instance a plan
// launches is a value of scan_inst.h (FsInst / LcInst), chosen in scan_plan.hip; DESIGN.md §4.1 "Which instance runs" has the table.
#pragma once
#include "common.h"
#include "pack_layout.h"
#include "scan_inst.h"

namespace ph {

constexpr int LC_NACC = 6;   // Σq, Σe, Σe·f1, Σe·f1·f2, Σd, count
constexpr int LC_MAX_SLOTS = 12;
// One launch per fused scan: every workgroup stores its partial words with device-scope stores, takes a ticket, and the workgroup that finishes LAST
// reads all partials (coalesced, every load independent), folds them in LDS into 128-bit sums (what merge_partials_kernel does as a second launch),
// stores them to out_lo / out_hi and, when mbox is set, into the mapped mailbox followed by the sequence number (what publish_kernel does as a
// third), and zeroes the ticket for the next launch. done == NULL: no tail (the caller launches the merge itself).
constexpr int SCAN_TAIL_MAX_ACC = 128;
struct ScanTail {
    unsigned *done;               // zero on entry, reset by the last workgroup
    unsigned long long *out_lo;   // [nacc]
    long long *out_hi;            // [nacc]
    int32_t nacc, min_stride;     // as launch_merge_partials
    unsigned long long *mbox;     // device address of the mailbox: lo[nacc] then hi[nacc]; NULL = no publish
    unsigned long long *flag;     // its sequence word
    unsigned long long seq;
};

// a column as its narrowed copy (ph_table::column::narrow): value = base + code, w bytes per code (1, 2 or 4)
struct ForCol {
    const uint8_t *data;
    int64_t base;
    int32_t w;
};

struct FilterSumProdParams {
    const int32_t *p0;  // int32 range-predicate column
    const int32_t *p2;  // int32 range-predicate column
    const int64_t *b;   // int64 range-predicate column, second factor of the product
    const int64_t *a;   // int64 first factor
    int32_t p0_lo, p0_hi, p2_lo, p2_hi;
    int64_t b_lo, b_hi;
    int64_t row_begin, row_end;
    long long *partials;  // [grid][2] = {Σ a*b, count}
    ScanTail tail;
    int32_t form;                         // ScanForm
    ForCol np0, np2, nb, na;              // FORM_NARROW*: the copies of p0, p2, b, a
    uint32_t np0_lo, np0_hi, np2_lo, np2_hi, nb_lo, nb_hi;   // the ranges over codes (lo > hi: nothing)
};

struct LowcardChainParams {
    const int32_t *p;   // int32 range-predicate column
    const int32_t *q;   // int32 summed column
    const int64_t *e, *d, *t;
    const uint8_t *k0, *k1;
    int32_t p_lo, p_hi;
    int32_t nk1;        // slot = k0 * nk1 + k1
    int32_t nslots;
    int64_t A1, B1, A2, B2;  // f1 = A1 + B1*d, f2 = A2 + B2*t
    int64_t row_begin, row_end;
    long long *partials;  // [grid][nslots][LC_NACC+1]: sums, count, first row id
    ScanTail tail;
    int32_t form;                 // ScanForm
    ForCol np, nq, ne, nd, nt;    // FORM_NARROW*: the copies of p, q, e, d, t (k0, k1 are read as they are)
    uint32_t np_lo, np_hi;        // the range over codes of p (lo > hi: nothing)
    int32_t lean;                 // FORM_NARROW32, |B1|, |B2| < 2^23 and not PH_SCAN_LEAN=0: the lean instance may run
    // lean: the factors over codes, f1 = A1c + B1c code_d with A1c = A1 + B1 nd.base (f2 alike), and ne.base; all exact in 32 bits
    int32_t A1c, B1c, A2c, B2c, e_base32;
    // the table's packed scan group once the plan has bound one (ph_scan_plan_run; lean plans only): one 64-bit word a row that holds the
    // codes of p, q, e, d, t and the slot k0 nk1 + k1, field f (PackField) at bit pk_shift[f], pk_width[f] bits wide, inside one dword.
    // NULL: none, the kernel reads the columns.
    const uint8_t *pk;
    uint8_t pk_shift[PACK_NFIELDS], pk_width[PACK_NFIELDS];
    int16_t bins;                 // this launch takes the bins body (written by ph_scan_plan_run from the chosen instance; nothing reads it)
    // the form of the group at pk (ScanGroupForm; written by bind_scan_group, read by the host's choice of instance only): SG_SPLIT56 is
    // pack_layout.h's blocks of 7168 bytes per 1024 rows, in lineitem's layout. bins and pk_form are 16 bits each only so that the struct,
    // and with it the kernels' argument segment and assembly, kept the size it had when bins was an int32_t alone; both are host-only facts
    // and may be widened freely by a change that accepts a new argument size.
    int16_t pk_form;
};

// the launch of instance `inst`; sw: the load form (nt) and the unroll of the instances that take them as template arguments
int launch_filter_sumprod(ph_ctx *ctx, const FilterSumProdParams &P, FsInst inst, const ScanSwitches &sw, int grid);
int launch_lowcard_chain(ph_ctx *ctx, const LowcardChainParams &P, LcInst inst, const ScanSwitches &sw, int grid);
// publish (may be NULL; ignored without a mailbox): the merge's last wave also publishes the merged words (ScanTail: done, nacc, mbox, flag, seq)
int launch_merge_partials(ph_ctx *ctx, const long long *partials, int nblocks, int nacc,
                          int min_stride, unsigned long long *out_lo, long long *out_hi, const ScanTail *publish = nullptr);

int launch_merge_partials_ops(ph_ctx *ctx, const long long *partials, int nblocks, int nacc, int stride,
                              unsigned long long opmask, unsigned long long *out_lo, long long *out_hi, const ScanTail *publish = nullptr);

}  // namespace ph
