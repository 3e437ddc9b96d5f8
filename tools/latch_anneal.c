// latch_anneal.c -- search a (round, lane) -> learned-triplet assignment for clatch_kernel that minimises LDS bank conflicts.
// C port and extension of tools/opt_latch_layout.py (which stays the generator of the geometry constants).
//
//   gcc -O2 -o tools/bin/latch_anneal tools/latch_anneal.c -lm
//   tools/bin/latch_anneal [switches] <mode> <rot> <swap> <iterations> <seed> [out.inc [b64 [copy shift mask [plan [keep plan [T0]]]]]]
//     --plain (default) / --merged: the conflict model the search minimises (see Model); both sums are printed and written for any table
//     --start table.inc: start from the LATCH_SLOT_TRIPLET_EX of a generated file (with 0 iterations: just evaluate it under both models)
//     --bases: the three movable copy bases are moves too, in steps of 4 bytes, inside what tests/test_latch_layout_table.py demands
//     --copy-bases b1 b2 b3: other bases than latch_layout.inc's;  --T0 t: starting temperature;  --note "text": a line for the file's header
//                            (where a --start table came from)
//     mode 0: any triplet in any slot (the kernel restores the descriptor bit order with ds_bpermute)
//     mode 1: lane l evaluates the eight triplets of ONE descriptor byte (its eight sign bits ARE that byte: no un-permute)
//     rot  1: a triplet may read its patch rows in the order 4..7, 0..3 (two base addresses per patch, same immediates)
//     swap 1: a triplet may exchange the roles of its a and c patches (S changes sign: the bit is then S > 0)
//     b64  1: a (round, kind) group whose 64 patch rows are all 8-byte aligned is costed as ONE access over 64 banks (ds_read_b64),
//             every other group as two dword accesses over 32 banks
//     plan:   the file tools/latch_plan_b64.py writes (copy shifts, the groups to keep aligned, a feasible assignment); keep plan 1 (default)
//             holds every planned group aligned throughout -- first the most aligned groups, then the fewest conflicts --, 0 starts from
//             the plan and minimises the modelled LDS cycles alone.  Measured on MI355X (profiles/clatch_two_paths.txt): the twelve-group
//             table makes the kernel SLOWER (conflict cycles x 2.1), so the shipped table is still the all-dword one of degree sum 71.
//
// Model (same as the Python tool): a wave's two 32-lane halves are banked independently, 32 banks x 4 B; every row step adds
// the same constant to all lanes' banks, so the conflict degree of a half-wave read is the largest multiplicity among the 32
// base banks of its patch kind; with rot the rotated lanes are 24 banks ahead during row steps 0..3 and 8 ahead during 4..7.
// Merged model (--merged): the LDS serves lanes that read the same address in one access (identical addresses broadcast), so the degree of a
// half-wave read of one patch kind is the largest number of DISTINCT addresses on one bank; the address is the patch's patch_addr under the
// slot's a <-> c exchange.  Equal patches of one kind then belong TOGETHER in a half-wave.  A group costed as ds_read_b64 keeps the plain rule.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define ROW0 5
#define COL0 5
#define STRIDE 56
static int COPY_BASE[4] = { 0, 3192, 6376, 9544 };   /* = latch_layout.inc (tools/opt_latch_layout.py choose_bases) */

static int pat[512][6];
static int bank[512][3];
static int pair64[512][3];        /* b64 model: (address / 8) mod 32 if the patch rows are 8-byte aligned, else -1 */
static int use_b64;                /* cost of a (round, kind) cell: every lane aligned -> one 64-bank access, else two 32-bank accesses */
static int copy_shift4[4];         /* per shifted copy: base moved by 4 bytes (flips which of its patches are 8-byte aligned) */
static int slot_t[8][64];          /* triplet in (round, lane) */
static int rot[512], swp[512];
static int mode, use_rot, use_swap;
static int use_merged;             /* --merged: lanes of a half-wave that read the SAME LDS address are served by one access (broadcast) */
static int addr[512][3];           /* patch_addr of the triplet's a, b, c patches */
static int have_plan, plan_flag[8][3];      /* planned (round, kind) cells that must stay all-aligned (hard constraint of the search) */
static int compatible(int n, int r)
{
    for (int k = 0; k < 3; ++k) if (plan_flag[r][k]) { const int kk = (swp[n] && k != 1) ? 2 - k : k; if (pair64[n][kk] < 0) return 0; }
    return 1;
}

static uint64_t rs = 88172645463325252ull;
static inline uint32_t rnd(void) { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 24); }
static inline double rndf(void) { return (rnd() & 0xFFFFFF) / 16777216.0; }

static int patch_addr(int row, int col)
{
    const int p = (row - ROW0) * STRIDE + (col - COL0);
    return COPY_BASE[p & 3] + 4 * copy_shift4[p & 3] + (p & ~3);
}

/* cost of half-wave group (round r, half h): sum over kind and row phase of 100 * max + sum of squares; *deg = sum of max */
static int round_aligned(int r, int k)      /* all 64 lanes of round r read kind k from 8-byte aligned rows */
{
    for (int l = 0; l < 64; ++l) { const int n = slot_t[r][l]; const int kk = (swp[n] && k != 1) ? 2 - k : k; if (pair64[n][kk] < 0) return 0; }
    return 1;
}
/* one more lane on bank b of a (kind, row phase) cell.  Plain model: every lane counts.  Merged model: a lane whose address another lane
   of the cell already reads is served by that lane's access, so only DISTINCT addresses count (key = address and row order). */
static inline void bank_insert(int* cnt, uint16_t (*seen)[32], int b, int key, int merged)
{
    if (merged) { for (int i = 0; i < cnt[b]; ++i) if (seen[b][i] == key) return; seen[b][cnt[b]] = (uint16_t)key; }
    cnt[b]++;
}
static int group_cost_model(int r, int h, int* deg, int merged)
{
    int cnt[3][2][32];
    uint16_t seen[3][2][32][32];
    memset(cnt, 0, sizeof cnt);
    int al[3] = { 0, 0, 0 }, nal[3] = { 0, 0, 0 };
    if (use_b64) for (int k = 0; k < 3; ++k) {
        al[k] = round_aligned(r, k);
        for (int l = 32 * h; l < 32 * h + 32; ++l) { const int n = slot_t[r][l]; const int kk = (swp[n] && k != 1) ? 2 - k : k; nal[k] += pair64[n][kk] >= 0; }
    }
    const int nph = use_rot ? 2 : 1;          /* without rotation the two row phases see the same banks: count one, weigh it twice */
    for (int l = 32 * h; l < 32 * h + 32; ++l) {
        const int n = slot_t[r][l];
        for (int k = 0; k < 3; ++k) {
            const int kk = (swp[n] && k != 1) ? 2 - k : k;
            const int b = al[k] ? pair64[n][kk] : bank[n][kk];
            const int key = 2 * addr[n][kk] + rot[n], m = merged && !al[k];      /* the b64 costing keeps its own rule */
            bank_insert(cnt[k][0], seen[k][0], (b + (rot[n] ? 24 : 0)) & 31, key, m);
            if (nph == 2) bank_insert(cnt[k][1], seen[k][1], (b + (rot[n] ? 8 : 0)) & 31, key, m);
        }
    }
    int c = 0, d = 0;
    for (int k = 0; k < 3; ++k)
        for (int ph = 0; ph < nph; ++ph) {
            int mx = 0, sq = 0;
            for (int b = 0; b < 32; ++b) { const int v = cnt[k][ph][b]; if (v > mx) mx = v; sq += v * v; }
            /* LDS cycles of this half-wave read, in half-steps: two 32-bank accesses, or one 64-bank access when the whole round is aligned */
            const int w = ((use_b64 && al[k]) ? 1 : 2) * (2 / nph);
            c += w * (100 * mx + sq); d += w * mx;
            /* search gradient towards homogeneous rounds: reward rounds that are nearly all-aligned (or nearly all-unaligned costs nothing) */
            if (use_b64 && !al[k]) c += (2 / nph) * 6 * (nal[k] > 16 ? 32 - nal[k] : 0);
        }
    if (deg) *deg = d;
    return c;
}
static int group_cost(int r, int h, int* deg) { return group_cost_model(r, h, deg, use_merged); }

/* sum over half-wave, kind, row phase of the largest bank multiplicity (x2: two row phases), whatever the read form;
   merged = 1 counts the DISTINCT addresses on a bank instead of the lanes */
static int total_deg_model(int merged)
{
    int t = 0;
    for (int r = 0; r < 8; ++r) for (int h = 0; h < 2; ++h) for (int k = 0; k < 3; ++k) {
        const int al = use_b64 && round_aligned(r, k);
        for (int ph = 0; ph < 2; ++ph) {
            int cnt[32]; uint16_t seen[32][32]; memset(cnt, 0, sizeof cnt);
            for (int l = 32 * h; l < 32 * h + 32; ++l) {
                const int n = slot_t[r][l]; const int kk = (swp[n] && k != 1) ? 2 - k : k;
                bank_insert(cnt, seen, ((al ? pair64[n][kk] : bank[n][kk]) + (rot[n] ? (ph ? 8 : 24) : 0)) & 31, 2 * addr[n][kk] + rot[n], merged && !al);
            }
            int mx = 0; for (int b = 0; b < 32; ++b) if (cnt[b] > mx) mx = cnt[b];
            t += mx;
        }
    }
    return t;
}
static int total_deg_plain(void) { return total_deg_model(0); }
static int total_deg_merged(void) { return total_deg_model(1); }
/* lanes of a half-wave whose patch read finds its address (and row order) already read by a lower lane of the same (round, kind) */
static int colocations(void)
{
    int t = 0;
    for (int r = 0; r < 8; ++r) for (int h = 0; h < 2; ++h) for (int k = 0; k < 3; ++k)
        for (int l = 32 * h; l < 32 * h + 32; ++l) {
            const int n = slot_t[r][l]; const int kk = (swp[n] && k != 1) ? 2 - k : k;
            for (int m = 32 * h; m < l; ++m) {
                const int n2 = slot_t[r][m]; const int kk2 = (swp[n2] && k != 1) ? 2 - k : k;
                if (addr[n][kk] == addr[n2][kk2] && rot[n] == rot[n2]) { ++t; break; }
            }
        }
    return t;
}
static void derive_banks(void)      /* everything that follows from the copy bases */
{
    for (int i = 0; i < 512; ++i) for (int k = 0; k < 3; ++k) {
        const int a = patch_addr(pat[i][2 * k], pat[i][2 * k + 1]);
        addr[i][k] = a; bank[i][k] = (a / 4) % 32; pair64[i][k] = (a & 7) ? -1 : (a / 8) % 32;
    }
}
#define WINDOW_BYTES (56 * STRIDE)
#define MAX_WAVE_BYTES 12688
static int bases_ok(void)           /* what tests/test_latch_layout_table.py demands of the four window copies */
{
    if (COPY_BASE[0] != 0) return 0;
    for (int k = 1; k < 4; ++k) if (COPY_BASE[k] < COPY_BASE[k - 1] + WINDOW_BYTES + 8) return 0;
    return COPY_BASE[3] + WINDOW_BYTES <= MAX_WAVE_BYTES;
}
double g_T0 = 60.0;
static int gcost[8][2];
static long total_cost(void) { long t = 0; for (int r = 0; r < 8; ++r) for (int h = 0; h < 2; ++h) t += gcost[r][h]; return t; }
static int total_deg2(void) { int t = 0; for (int r = 0; r < 8; ++r) for (int h = 0; h < 2; ++h) { int d; group_cost(r, h, &d); t += d; } return t; }

int main(int argc, char** argv)
{
    const char* start_path = NULL; const char* note = NULL; int move_bases = 0;
    static char cmdline[2048];          /* the command line as given, for the generated file's header (the output path aside) */
    for (int i = 0, pos = 0; i < argc; ++i) {
        const char* a = (i > 0 && strstr(argv[i], ".inc") && strcmp(argv[i - 1], "--start")) ? "<this file>" : argv[i];
        if (i > 0 && !strcmp(argv[i - 1], "--note")) a = "...";
        if (pos + (int)strlen(a) + 2 < (int)sizeof cmdline) pos += sprintf(cmdline + pos, " %s", a);
    }
    {   /* switches may stand anywhere; what remains is the positional command line */
        int na = 1;
        for (int i = 1; i < argc; ++i) {
            if (!strcmp(argv[i], "--merged")) use_merged = 1;
            else if (!strcmp(argv[i], "--plain")) use_merged = 0;
            else if (!strcmp(argv[i], "--bases")) move_bases = 1;
            else if (!strcmp(argv[i], "--start") && i + 1 < argc) start_path = argv[++i];
            else if (!strcmp(argv[i], "--T0") && i + 1 < argc) g_T0 = atof(argv[++i]);
            else if (!strcmp(argv[i], "--note") && i + 1 < argc) note = argv[++i];
            else if (!strcmp(argv[i], "--copy-bases") && i + 3 < argc) { for (int k = 1; k < 4; ++k) COPY_BASE[k] = atoi(argv[++i]); }
            else argv[na++] = argv[i];
        }
        argc = na;
    }
    if (argc < 6) { fprintf(stderr, "usage: %s [--merged|--plain] [--start table.inc] [--bases] [--copy-bases b1 b2 b3] [--T0 t] mode rot swap iterations seed [out] [b64] [copy shift mask]\n", argv[0]); return 2; }
    if (!bases_ok()) { fprintf(stderr, "copy bases: gaps or wave bytes out of range\n"); return 1; }
    mode = atoi(argv[1]); use_rot = atoi(argv[2]); use_swap = atoi(argv[3]);
    use_b64 = argc > 7 ? atoi(argv[7]) : 0;
    if (argc > 8) for (int k = 0; k < 4; ++k) copy_shift4[k] = (atoi(argv[8]) >> k) & 1;
    const long iters = atol(argv[4]); rs ^= (uint64_t)atol(argv[5]) * 0x9E3779B97F4A7C15ull;
    const char* pattern_path = "coloc_amd/csrc/latch_pattern.inc";
    FILE* f = fopen(pattern_path, "r");
    if (!f) { perror(pattern_path); return 1; }
    char line[256]; int n = 0;
    while (fgets(line, sizeof line, f))
        if (line[0] == '{' && n < 512 && sscanf(line, "{%d,%d, %d,%d, %d,%d}", &pat[n][0], &pat[n][1], &pat[n][2], &pat[n][3], &pat[n][4], &pat[n][5]) == 6) ++n;
    fclose(f);
    if (n != 512) { fprintf(stderr, "pattern: %d rows\n", n); return 1; }
    derive_banks();
    /* start: mode 0 natural order (triplet 64 r + l); mode 1 lane l <- byte l, round j <- bit j of the byte */
    for (int r = 0; r < 8; ++r) for (int l = 0; l < 64; ++l) slot_t[r][l] = mode ? 8 * l + r : 64 * r + l;
    if (argc > 9) {       /* a planned start (tools/latch_plan_b64.py): copy shifts, the cells to keep aligned, a feasible assignment */
        FILE* pf = fopen(argv[9], "r");
        if (!pf) { perror(argv[9]); return 1; }
        int shm = 0;
        if (fscanf(pf, "%d", &shm) != 1) return 1;
        for (int k = 0; k < 4; ++k) copy_shift4[k] = (shm >> k) & 1;
        derive_banks();
        for (int r = 0; r < 8; ++r) if (fscanf(pf, "%d %d %d", &plan_flag[r][0], &plan_flag[r][1], &plan_flag[r][2]) != 3) return 1;
        for (int r = 0; r < 8; ++r) for (int l = 0; l < 64; ++l) { int v; if (fscanf(pf, "%d", &v) != 1) return 1; slot_t[r][l] = v & 511; swp[v & 511] = (v >> 10) & 1; }
        fclose(pf);
        have_plan = argc > 10 ? atoi(argv[10]) : 1; use_b64 = 1;      /* argv[10] = 0: the plan is only the starting point */
        for (int r = 0; r < 8; ++r) for (int l = 0; l < 64; ++l) if (!compatible(slot_t[r][l], r)) { fprintf(stderr, "plan: slot (%d, %d) incompatible\n", r, l); return 1; }
        if (argc > 11) { const double t0 = atof(argv[11]); if (t0 > 0) { extern double g_T0; g_T0 = t0; } }
    }
    if (start_path) {     /* start from a written table: the LATCH_SLOT_TRIPLET_EX of a generated file (iterations 0 just evaluates it) */
        FILE* sf = fopen(start_path, "r");
        if (!sf) { perror(start_path); return 1; }
        int in = 0, ns = 0;
        while (fgets(line, sizeof line, sf)) {
            if (!in) { in = strstr(line, "#define LATCH_SLOT_TRIPLET_EX") != NULL; continue; }
            for (char* q = line; *q && ns < 512; ) {
                if (*q < '0' || *q > '9') { ++q; continue; }
                const int v = (int)strtol(q, &q, 10);
                slot_t[ns >> 6][ns & 63] = v & 511; rot[v & 511] = (v >> 9) & 1; swp[v & 511] = (v >> 10) & 1; ++ns;
            }
            if (!strchr(line, '\\')) break;
        }
        fclose(sf);
        if (ns != 512) { fprintf(stderr, "%s: %d slots\n", start_path, ns); return 1; }
    }
    for (int r = 0; r < 8; ++r) for (int h = 0; h < 2; ++h) gcost[r][h] = group_cost(r, h, NULL);
    printf("start: degree sum %.1f (x2: %d)\n", total_deg2() / 2.0, total_deg2());
    double T = g_T0; const double cool = pow(0.4 / g_T0, 1.0 / (double)iters);
    long cur = total_cost(), best = cur;
    static int best_slot[8][64], best_rot[512], best_swp[512], best_base[4];
    memcpy(best_base, COPY_BASE, sizeof best_base);
    memcpy(best_slot, slot_t, sizeof slot_t); memcpy(best_rot, rot, sizeof rot); memcpy(best_swp, swp, sizeof swp);
    for (long it = 0; it < iters; ++it, T *= cool) {
        const uint32_t kind = rnd() % 16;
        int touched[4][2], nt = 0;
        int r1 = 0, l1 = 0, r2 = 0, l2 = 0, tn = -1, what = 0, bk = 0, bd = 0;
        if (move_bases && (rnd() & 4095) == 0) {       /* one shifted copy moves by 4 bytes: every patch of that copy one bank on */
            bk = 1 + rnd() % 3; bd = (rnd() & 1) ? 4 : -4;
            COPY_BASE[bk] += bd;
            if (!bases_ok()) { COPY_BASE[bk] -= bd; continue; }
            COPY_BASE[bk] -= bd;
            what = 5;
        } else if (kind < 10 || (!use_rot && !use_swap)) {
            if (mode == 0) {                     /* swap two slots */
                r1 = rnd() & 7; l1 = rnd() & 63; r2 = rnd() & 7; l2 = rnd() & 63;
                if (r1 == r2 && (l1 >> 5) == (l2 >> 5)) continue;
                what = 1;
            } else if (rnd() & 1) {              /* two rounds of one lane */
                l1 = l2 = rnd() & 63; r1 = rnd() & 7; r2 = rnd() & 7;
                if (r1 == r2) continue;
                what = 1;
            } else {                             /* the bytes of two lanes (all eight rounds) */
                l1 = rnd() & 63; l2 = rnd() & 63;
                if ((l1 >> 5) == (l2 >> 5)) continue;      /* same half-wave: no effect on the cost */
                what = 2;
            }
        } else {
            tn = rnd() & 511;
            what = (use_rot && (!use_swap || (rnd() & 1))) ? 3 : 4;
        }
        long d = 0;
        if (have_plan) {          /* keep every planned cell aligned */
            if (what == 1 && (!compatible(slot_t[r1][l1], r2) || !compatible(slot_t[r2][l2], r1))) continue;
            if (what == 4) {
                int rr = -1; for (int r = 0; r < 8 && rr < 0; ++r) for (int l = 0; l < 64; ++l) if (slot_t[r][l] == tn) { rr = r; break; }
                swp[tn] ^= 1; const int ok = compatible(tn, rr); swp[tn] ^= 1;
                if (!ok) continue;
            }
        }
        if (what == 1) {
            int t = slot_t[r1][l1]; slot_t[r1][l1] = slot_t[r2][l2]; slot_t[r2][l2] = t;
            touched[nt][0] = r1; touched[nt++][1] = l1 >> 5;
            if (r2 != r1 || (l2 >> 5) != (l1 >> 5)) { touched[nt][0] = r2; touched[nt++][1] = l2 >> 5; }
        } else if (what == 2) {
            for (int r = 0; r < 8; ++r) { int t = slot_t[r][l1]; slot_t[r][l1] = slot_t[r][l2]; slot_t[r][l2] = t; }
        } else if (what == 3) rot[tn] ^= 1;
        else if (what == 5) { COPY_BASE[bk] += bd; derive_banks(); }
        else swp[tn] ^= 1;
        int newc[8][2]; int chg[8][2]; memset(chg, 0, sizeof chg);
        if (what == 1) { for (int i = 0; i < nt; ++i) { chg[touched[i][0]][touched[i][1]] = 1; if (use_b64) chg[touched[i][0]][touched[i][1] ^ 1] = 1; } }
        else if (what == 2 || what == 5) { for (int r = 0; r < 8; ++r) chg[r][0] = chg[r][1] = 1; }
        else { for (int r = 0; r < 8; ++r) for (int l = 0; l < 64; ++l) if (slot_t[r][l] == tn) { chg[r][l >> 5] = 1; if (use_b64) chg[r][(l >> 5) ^ 1] = 1; } }
        for (int r = 0; r < 8; ++r) for (int h = 0; h < 2; ++h) if (chg[r][h]) { newc[r][h] = group_cost(r, h, NULL); d += newc[r][h] - gcost[r][h]; }
        if (d <= 0 || rndf() < exp(-(double)d / T)) {
            for (int r = 0; r < 8; ++r) for (int h = 0; h < 2; ++h) if (chg[r][h]) gcost[r][h] = newc[r][h];
            cur += d;
            if (cur < best) { best = cur; memcpy(best_base, COPY_BASE, sizeof best_base); memcpy(best_slot, slot_t, sizeof slot_t); memcpy(best_rot, rot, sizeof rot); memcpy(best_swp, swp, sizeof swp); }
        } else {   /* undo */
            if (what == 1) { int t = slot_t[r1][l1]; slot_t[r1][l1] = slot_t[r2][l2]; slot_t[r2][l2] = t; }
            else if (what == 2) { for (int r = 0; r < 8; ++r) { int t = slot_t[r][l1]; slot_t[r][l1] = slot_t[r][l2]; slot_t[r][l2] = t; } }
            else if (what == 3) rot[tn] ^= 1;
            else if (what == 5) { COPY_BASE[bk] -= bd; derive_banks(); }
            else swp[tn] ^= 1;
        }
    }
    memcpy(COPY_BASE, best_base, sizeof best_base); derive_banks();
    memcpy(slot_t, best_slot, sizeof slot_t); memcpy(rot, best_rot, sizeof rot); memcpy(swp, best_swp, sizeof swp);
    const int d2 = total_deg2();
    int nrot = 0, nswp = 0; for (int i = 0; i < 512; ++i) { nrot += rot[i]; nswp += swp[i]; }
    int nb64 = 0; if (use_b64) for (int r = 0; r < 8; ++r) for (int k = 0; k < 3; ++k) nb64 += round_aligned(r, k);
    printf("plain degree sum %.1f, merged degree sum %.1f, same-address co-locations %d (the search minimised the %s model)\n",
           total_deg_plain() / 2.0, total_deg_merged() / 2.0, colocations(), use_merged ? "merged" : "plain");
    printf("copy bases { %d, %d, %d, %d }%s\n", COPY_BASE[0], COPY_BASE[1], COPY_BASE[2], COPY_BASE[3], move_bases ? " (bases were moves of the search)" : "");
    printf("mode %d rot %d swap %d b64 %d shift %d%d%d%d: %s %.1f (today's layout: 162 half-steps = degree sum 81; bound 48), %d rotated, %d swapped, %d of 24 (round, kind) reads as ds_read_b64\n",
           mode, use_rot, use_swap, use_b64, copy_shift4[0], copy_shift4[1], copy_shift4[2], copy_shift4[3], use_b64 ? "LDS half-steps / 2" : "degree sum", d2 / (use_b64 ? 4.0 : 2.0), nrot, nswp, nb64);
    if (argc > 6) {
        FILE* o = fopen(argv[6], "w");
        if (!o) { perror(argv[6]); return 1; }
        fprintf(o, "// GENERATED by tools/latch_anneal.c; command line:%s", cmdline);
        if (note) fprintf(o, "\n// %s", note);
        fprintf(o, "\n// (mode %d rot %d swap %d, %ld iterations, seed %s)  sum of half-wave conflict degrees: plain model %.1f, merged model %.1f (lower bound 48);\n"
                   "// %d same-address co-locations.  The search minimised the %s model (plain: every lane on a bank counts; merged: lanes of a half-wave that\n"
                   "// read the same LDS address are one access, so only distinct addresses on a bank count).  Copy bases { %d, %d, %d, %d }",
                mode, use_rot, use_swap, iters, argv[5], total_deg_plain() / 2.0, total_deg_merged() / 2.0, colocations(), use_merged ? "MERGED" : "PLAIN",
                COPY_BASE[0], COPY_BASE[1], COPY_BASE[2], COPY_BASE[3]);
        if (use_b64) fprintf(o, "; %d of 24 (round, kind) groups 8-byte aligned; modelled LDS cycles of the 48 half-wave group reads %.1f (two per\n// dword-pair access, one per aligned 8-byte access over 64 banks)", nb64, d2 / 2.0);
        fprintf(o, ".\n");
        fprintf(o, "// slot = round*64 + lane evaluates learned triplet (v & 511); bit 9: rows in the order 4..7,0..3; bit 10: the slot reads the triplet's a and c\n// patches in exchanged roles (it then computes -S, and its descriptor bit is S' > 0 instead of S < 0).  Geometry constants: latch_layout.inc;\n// LATCH_COPY_SHIFT4[k] = 1: shifted copy k starts 4 bytes behind LATCH_COPY_BASES[k], which turns its 8-byte aligned patch rows into the other half.\n// LATCH_ROUND_B64[r] = {a, b, c}: all 64 lanes of round r read that patch kind from 8-byte aligned rows (tests/test_latch_layout_table.py recomputes it).\n");
        fprintf(o, "#define LATCH_DEGREE_PLAIN %g\n#define LATCH_DEGREE_MERGED %g\n#define LATCH_COLOCATIONS %d\n", total_deg_plain() / 2.0, total_deg_merged() / 2.0, colocations());
        fprintf(o, "#define LATCH_COPY_SHIFT4 { %d, %d, %d, %d }\n", copy_shift4[0], copy_shift4[1], copy_shift4[2], copy_shift4[3]);
        fprintf(o, "#define LATCH_ROUND_B64 { \\\n");
        for (int r = 0; r < 8; ++r) fprintf(o, "    { %d, %d, %d }, \\\n", use_b64 ? round_aligned(r, 0) : 0, use_b64 ? round_aligned(r, 1) : 0, use_b64 ? round_aligned(r, 2) : 0);
        fprintf(o, "}\n");
        fprintf(o, "#define LATCH_SLOT_TRIPLET_EX { \\\n");
        for (int r = 0; r < 8; ++r) for (int l = 0; l < 64; l += 16) {
            fprintf(o, "   ");
            for (int i = 0; i < 16; ++i) { const int t = slot_t[r][l + i]; fprintf(o, " %d,", t | (rot[t] << 9) | (swp[t] << 10)); }
            fprintf(o, " \\\n");
        }
        fprintf(o, "}\n");
        fclose(o);
    }
    return 0;
}
