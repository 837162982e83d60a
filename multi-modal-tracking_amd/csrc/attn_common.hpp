// Shared by the MAM attention translation units (attention.hip, attention_ps.hip): the query-block
// geometry and the asymmetric key mapping (MamBlock / MamKeys: which keys a query block sees), the XCD-aware block
// map, LDS-DMA issue / counted waits, and the LDS fragment reads.
#pragma once
#include "common.hpp"

// MMT_ATTN_CHECK=1 builds turn the key-tile index checks into device asserts
#ifndef MMT_ATTN_CHECK
#define MMT_ATTN_CHECK 0
#endif
#if MMT_ATTN_CHECK
#include <cassert>
#define MMT_ATTN_ASSERT(c) assert(c)
#else
#define MMT_ATTN_ASSERT(c) ((void)0)
#endif

namespace {

constexpr int D = 64, KB = 64;                 // head dim, keys per K / V tile
constexpr int FQ = 128, FTILE = 2 * KB * 128;  // queries per throughput workgroup; bytes of a K + V tile slot
constexpr float LZ_LO = 0x1p-100f, LZ_HI = 0x1p100f;  // range of the row sums without a reference point

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int N>
struct attn_ic {
    static constexpr int value = N;
};

// XCD-aware bijective block remap (as gemm.hip): workgroups are dealt round-robin over the 8 XCDs, so
// consecutive (query block, head, sequence) ids would put the query blocks of one (sequence, head) on
// different XCDs, each fetching the same K / V rows into its own L2.  Giving each XCD a contiguous run
// of ids (query block fastest) keeps those re-reads in one L2.  Speed only.
// SMALL_GRIDS = false: grids that fit the chip (<= 256 workgroups, batch-1 tracking) keep the identity
// map (B = 8 / 32 throughput kernel 33 -> 29 / 90 -> 84 us with the remap; the single-wave batch-1 grid
// gains nothing); true: remapped at every grid size (the range-checked kernels).
template <bool SMALL_GRIDS>
MMT_DEV void attn_block_ids(int& bx, int& by, int& bz) {
    const int nbx = gridDim.x, nby = gridDim.y, nwg = nbx * nby * gridDim.z;
    if constexpr (!SMALL_GRIDS) {
        if (nwg <= 256) {
            bx = blockIdx.x;
            by = blockIdx.y;
            bz = blockIdx.z;
            return;
        }
    }
    const int orig = blockIdx.x + nbx * (blockIdx.y + nby * blockIdx.z);
    const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int lin = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
    bx = lin % nbx;
    by = (lin / nbx) % nby;
    bz = lin / (nbx * nby);
}

template <int N>
MMT_DEV void attn_wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
typedef __attribute__((address_space(3))) void attn_lds_void;
typedef __attribute__((address_space(1))) void attn_glb_void;
MMT_DEV void attn_glds16(const void* src, char* dst) {
    __builtin_amdgcn_global_load_lds((attn_glb_void*)src, (attn_lds_void*)dst, 16, 0, 0);
}
// ds_read_b64_tr_b16 as inline asm: through the builtin, hipcc cannot tell the read from the
// in-flight LDS-DMA writes and drains vmcnt(0) before it (i.e. waits for the whole prefetch ring).
// Inline asm is invisible to its wait-count tracking, so the caller waits with attn_lds_wait().
template <int OFF>
MMT_DEV uint2 attn_tr16(const char* p) {
    uint2 r;
    const uint32_t a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(a), "n"(OFF));
    return r;
}
MMT_DEV void attn_lds_wait() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);  // keep the MFMAs that consume the asm reads below the wait
}

MMT_DEV void attn_wait_dyn(int n) {
    switch (n) {
        case 0: attn_wait_vm<0>(); break;
        case 1: attn_wait_vm<1>(); break;
        case 2: attn_wait_vm<2>(); break;
        case 3: attn_wait_vm<3>(); break;
        case 4: attn_wait_vm<4>(); break;
        case 5: attn_wait_vm<5>(); break;
        case 6: attn_wait_vm<6>(); break;
        case 7: attn_wait_vm<7>(); break;
        case 8: attn_wait_vm<8>(); break;
        case 9: attn_wait_vm<9>(); break;
        case 10: attn_wait_vm<10>(); break;
        case 11: attn_wait_vm<11>(); break;
        case 12: attn_wait_vm<12>(); break;
        case 13: attn_wait_vm<13>(); break;
        case 14: attn_wait_vm<14>(); break;
        case 15: attn_wait_vm<15>(); break;
        case 16: attn_wait_vm<16>(); break;
        case 17: attn_wait_vm<17>(); break;
        default: attn_wait_vm<18>(); break;
    }
}

// first out row of query q of sequence s (mmt_attn_params.out_pitch / out_q0: compact activations of the
// template K/V cache passes; identity layout by default)
MMT_DEV int64_t attn_out_row(const mmt_attn_params& p, int s, int q, int64_t pitch) {
    return (int64_t)s * (p.out_pitch > 0 ? p.out_pitch : pitch) + q - p.out_q0;
}

// V image swizzle: chunk c of row r at c ^ (r & 6) ^ ((r & 2) << 1): the 4 rows x 4 chunks a
// half-wave reads per tr instruction then cover all 64 banks once.
MMT_DEV int attn_vswz(int row) { return (row & 6) ^ ((row & 2) << 1); }

// The keys one query of sequence s sees, and where they live.  Rows of qkv are rs = 3 C elements
// (q | k | v), sequences are pitch rows apart.  cross = false: key kk is the sequence's own token kk.
// cross = true (search queries of the cross-modal form): the asymmetric stream [template V | template I |
// own search], i.e. keys [0, n_t) are the template of the RGB sequence sV = s % Bm, [n_t, 2 n_t) the
// template of the TIR sequence sI = sV + Bm, and [2 n_t, ntok + n_t) the own search tokens n_t .. ntok - 1.
// Row pointers are to the row's start: callers add the k / v and head offsets.
// (A base of MamBlock, not part of it: merged into one struct the kernels compile to different code.)
// TL = true (mmt_mam_attention_tl): every sequence has its own count of valid template rows, tl <= n_t.
// n_t is then the length of the block's own sequence and nV / nI those of sV / sI, the stream is that of a
// launch with those lengths, and the rows stay where they are: search rows start at row np (the launch's
// n_t).  TL = false keeps the code below as it was, statement for statement.
template <typename T, bool TL = false>
struct MamKeys {
    const T* qkv;
    int64_t pitch, rs;
    int n_t, s, sV, sI;
    bool cross;
    int np, nV, nI;  // TL only
    MMT_DEV const T* key_row(int kk) const {
        int seq = s, row = kk;
        if constexpr (TL) {
            if (cross) {
                if (kk < nV) seq = sV;
                else if (kk < nV + nI) { seq = sI; row = kk - nV; }
                else row = kk - nV - nI + np;
            } else if (kk >= n_t) row = kk - n_t + np;
        } else if (cross) {
            if (kk < n_t) seq = sV;
            else if (kk < 2 * n_t) { seq = sI; row = kk - n_t; }
            else row = kk - n_t;
        }
        return qkv + ((int64_t)seq * pitch + row) * rs;
    }
};

// One query block of the MAM: QB consecutive queries [q0, min(q0 + QB, qend)) of sequence s, all template
// or all search tokens, and the Lk keys they see.  This is the one statement of that geometry for the
// forward kernels of attention.hip (attention_ps.hip's item walk and attention_bwd.hip's joint-key decode
// keep their own forms).  Query blocks are numbered template blocks first (ceil(n_t / QB) of them, the
// last one short), then search blocks from token n_t; q_part = 2 launches start at the first search
// block.  Template queries see the sequence's own template keys (Lk = n_t); search queries see every own
// token (Lk = ntok) or, cross-modal (p.asym), the stream of MamKeys (Lk = ntok + n_t).  Keys are consumed
// in nkt() tiles of KB; the last may be short.
// TL = true: place() takes the lengths int32[S]; the grid and the block numbering are the launch's (n_t
// rows of template blocks), a block is live when its sequence's lengths are in 1..n_t and, for a template
// block, when it starts below tl.  The kernels return on a dead block before any DMA, barrier or store; the
// decision is the same for every thread of the workgroup.  The kernels take the lengths as a parameter pack
// (TLEN...: empty, or one const int32_t*), so that the launches without lengths keep their kernel arguments
// and their code; attn_has_len names which form a pack selects.
template <typename... TLEN>
constexpr bool attn_has_len = sizeof...(TLEN) == 1;
template <typename T, int QB, bool TL = false>
struct MamBlock : MamKeys<T, TL> {
    int ntok, nqb_t, q0, qend, Lk;
    bool tmpl;
    bool live;  // TL only
    MMT_DEV MamBlock(const mmt_attn_params& p, int bx, int s) : MamBlock(p) { place(p, bx, s); }
    MMT_DEV MamBlock(const mmt_attn_params& p, int bx, int s, const int32_t* tlen) : MamBlock(p) { place(p, bx, s, tlen); }
    // The same in two steps, the launch-only part first and the block's place after the kernel has read its
    // block ids (impl 17 / 21 is written in that order and its generated code depends on it); the block
    // is valid after place().
    MMT_DEV explicit MamBlock(const mmt_attn_params& p) {
        this->n_t = p.n_t;
        ntok = p.ntok;
        this->pitch = p.tok_pitch > 0 ? p.tok_pitch : ntok;
        nqb_t = (this->n_t + QB - 1) / QB;
    }
    MMT_DEV void place(const mmt_attn_params& p, int bx, int s) {
        const int n_t = this->n_t;
        this->s = s;
        const int qb = bx + (p.q_part == 2 ? nqb_t : 0);
        tmpl = qb < nqb_t;
        q0 = tmpl ? qb * QB : n_t + (qb - nqb_t) * QB;
        qend = tmpl ? n_t : ntok;
        Lk = tmpl ? n_t : (p.asym ? ntok + n_t : ntok);
        this->cross = p.asym && !tmpl;
        this->rs = 3 * (int64_t)p.C;
        this->qkv = (const T*)p.qkv;
        this->sV = s % p.Bm;
        this->sI = this->sV + p.Bm;
    }
    MMT_DEV void place(const mmt_attn_params& p, int bx, int s, const int32_t* tlen) {
        static_assert(TL, "lengths belong to the TL form");
        place(p, bx, s);
        const int np = p.n_t, tl = tlen[s], tV = p.asym ? tlen[this->sV] : tl, tI = p.asym ? tlen[this->sI] : tl;
        this->np = np;
        this->n_t = tl;
        this->nV = tV;
        this->nI = tI;
        live = tl >= 1 && tl <= np && (tmpl ? q0 < tl : (tV >= 1 && tV <= np && tI >= 1 && tI <= np));
        if (tmpl) qend = tl;
        Lk = tmpl ? tl : ntok - np + (p.asym ? tV + tI : tl);
    }
    MMT_DEV int nkt() const { return (Lk + KB - 1) / KB; }
    // no full key tile straddles two key segments
    MMT_DEV bool aligned() const {
        if constexpr (TL) return (this->n_t | this->nV | this->nI) % KB == 0;
        else return this->n_t % KB == 0;
    }
    // query q, clamped to the block's last query (rows past it are staged and computed, never stored)
    MMT_DEV const T* q_row(int q) const { return this->qkv + ((int64_t)this->s * this->pitch + min(q, qend - 1)) * this->rs; }
};

// LDS-DMA of one 1-KiB piece of a query block's Q image: query rows 8 piece .. 8 piece + 7 of the block
// (rows past the block's end re-read its last query), 128 B per row at head h, chunk c of row r stored at
// c ^ (r & 7); this lane moves chunk pcol of row prow.  (One piece per call: the piece loops stay in the
// kernels, where moving them into a helper changes the generated code.)
template <typename T, int QB, bool TL>
MMT_DEV void attn_issue_q(const MamBlock<T, QB, TL>& blk, int h, char* qimg, int piece, int prow, int pcol) {
    const int r = piece * 8 + prow;
    const T* src = blk.q_row(blk.q0 + r) + h * D;
    attn_glds16(src + ((pcol ^ prow) * 8), qimg + piece * 1024);
}

}  // namespace
