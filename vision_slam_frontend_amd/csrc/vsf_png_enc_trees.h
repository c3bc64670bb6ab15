// vsf_png_enc_trees.h -- what zlib 1.2.11 does with ONE deflate block once its symbols are known, restated step by step
// (trees.c: build_tree with pqdownheap's depth tie-break, gen_bitlen with its overflow repair, gen_codes, scan_tree, build_bl_tree,
// _tr_flush_block's choice between a stored, a static and a dynamic block, send_all_trees), and deflate_rle's greedy parse in closed
// form.  Serial code for one lane; k_png_enc.hip runs it on the device, vsf_png_enc_host.cc on the CPU (the model the CPU tests
// compare with the real library), so both are the same text.
#ifndef VSF_PNG_ENC_TREES_H_
#define VSF_PNG_ENC_TREES_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define VSF_PE_HD __host__ __device__ inline
#else
#define VSF_PE_HD inline
#endif

#define VSF_PE_L_CODES 286
#define VSF_PE_D_CODES 30
#define VSF_PE_BL_CODES 19
#define VSF_PE_HEAP (2 * VSF_PE_L_CODES + 1)
#define VSF_PE_HDR_WORDS 80  // 3 + 14 + 19 * 3 + 316 * 7 bits at most = 2286 bits

// deflate_rle at offset k of a run of L equal bytes: 0 no symbol starts here, 1 a literal, >= 3 a match of that length (distance 1).
// The run's first byte is a literal; behind it come matches of min(258, rest) while at least 3 bytes remain, then literals.
VSF_PE_HD uint32_t vsf_pe_symbol(uint32_t k, uint32_t L) {
  if (k == 0) return 1;
  const uint32_t j = k - 1, q = j / 258u, m = j - q * 258u;
  uint32_t len = (L - 1) - q * 258u;
  if (len > 258u) len = 258u;
  if (len >= 3u) return m == 0 ? len : 0;
  return 1;
}

// length - 3 (0 .. 255) -> length code 0 .. 28 (symbol 257 + code), its extra bits and their value
VSF_PE_HD int vsf_pe_length_code(uint32_t lc, int* extra, uint32_t* value) {
  if (lc < 8) {
    *extra = 0;
    *value = 0;
    return (int)lc;
  }
  if (lc == 255) {
    *extra = 0;
    *value = 0;
    return 28;
  }
  int e = 1;
  while ((lc >> (e + 3)) != 0) e++;  // floor(log2(lc)) - 2
  *extra = e;
  *value = lc & ((1u << e) - 1u);
  return 4 * e + 4 + (int)((lc >> e) & 3u);
}

VSF_PE_HD int vsf_pe_static_llen(int n) { return n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8; }
VSF_PE_HD uint32_t vsf_pe_reverse(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; i++) {
    r = (r << 1) | (code & 1u);
    code >>= 1;
  }
  return r;
}
// the static literal/length code of symbol n, reversed for an LSB-first stream
VSF_PE_HD uint32_t vsf_pe_static_lcode(int n) {
  const uint32_t c = n < 144 ? 0x30u + n : n < 256 ? 0x190u + (n - 144) : n < 280 ? (uint32_t)(n - 256) : 0xC0u + (n - 280);
  return vsf_pe_reverse(c, vsf_pe_static_llen(n));
}

enum { VSF_PE_TREE_L = 0, VSF_PE_TREE_D = 1, VSF_PE_TREE_BL = 2 };

struct VsfPeWork {
  // one tree at a time (ct_data's Freq / Dad / Len and the heap of deflate_state)
  uint16_t freq[VSF_PE_HEAP], dad[VSF_PE_HEAP], len[VSF_PE_HEAP + 1], heap[VSF_PE_HEAP + 1];
  uint8_t depth[VSF_PE_HEAP];
  uint16_t bl_count[16];
  // what is kept of each
  uint16_t llen[VSF_PE_L_CODES + 1], lcode[VSF_PE_L_CODES];
  uint16_t dlen[VSF_PE_D_CODES + 1], dcode[VSF_PE_D_CODES];
  uint16_t bllen[VSF_PE_BL_CODES + 1], blcode[VSF_PE_BL_CODES], blfreq[VSF_PE_BL_CODES];
  int l_max, d_max, max_blindex;
  uint32_t opt_len, static_len;  // bits (a block holds at most 16383 symbols of at most 33 bits)
};

struct VsfPePlan {
  uint32_t type;       // 0 stored, 1 static, 2 dynamic
  uint32_t hdr_bits;   // bits of hdr: the block's three header bits and, dynamic, the trees
  uint32_t body_bits;  // bits of the block behind its first three (stored: LEN, NLEN and the bytes, the padding not counted)
  uint32_t pad_;
  uint32_t lcode[VSF_PE_L_CODES];  // code (reversed) | length << 16
  uint32_t dcode0;
  uint32_t hdr[VSF_PE_HDR_WORDS];
};

VSF_PE_HD bool vsf_pe_smaller(const VsfPeWork& s, int n, int m) {
  return s.freq[n] < s.freq[m] || (s.freq[n] == s.freq[m] && s.depth[n] <= s.depth[m]);
}

VSF_PE_HD void vsf_pe_downheap(VsfPeWork& s, int heap_len, int k) {
  const int v = s.heap[k];
  int j = k << 1;
  while (j <= heap_len) {
    if (j < heap_len && vsf_pe_smaller(s, s.heap[j + 1], s.heap[j])) j++;
    if (vsf_pe_smaller(s, v, s.heap[j])) break;
    s.heap[k] = s.heap[j];
    k = j;
    j <<= 1;
  }
  s.heap[k] = (uint16_t)v;
}

VSF_PE_HD int vsf_pe_extra_bits(int which, int n) {
  if (which == VSF_PE_TREE_L) return n < 257 + 8 || n == 257 + 28 ? 0 : ((n - 257) >> 2) - 1;
  if (which == VSF_PE_TREE_D) return n < 4 ? 0 : (n >> 1) - 1;
  return n == 16 ? 2 : n == 17 ? 3 : n == 18 ? 7 : 0;
}

// build_tree + gen_bitlen + gen_codes over s.freq[0 .. elems): lengths into s.len, codes (reversed) into `code`; -> max_code.
VSF_PE_HD int vsf_pe_build_tree(VsfPeWork& s, int which, uint16_t* code) {
  const int elems = which == VSF_PE_TREE_L ? VSF_PE_L_CODES : which == VSF_PE_TREE_D ? VSF_PE_D_CODES : VSF_PE_BL_CODES;
  const int max_length = which == VSF_PE_TREE_BL ? 7 : 15;
  int heap_len = 0, heap_max = VSF_PE_HEAP, max_code = -1;
  for (int n = 0; n < elems; n++) {
    if (s.freq[n] != 0) {
      s.heap[++heap_len] = (uint16_t)(max_code = n);
      s.depth[n] = 0;
    } else {
      s.len[n] = 0;
    }
  }
  while (heap_len < 2) {
    const int node = s.heap[++heap_len] = (uint16_t)(max_code < 2 ? ++max_code : 0);
    s.freq[node] = 1;
    s.depth[node] = 0;
    s.opt_len--;
    if (which == VSF_PE_TREE_L) s.static_len -= (uint32_t)vsf_pe_static_llen(node);
    if (which == VSF_PE_TREE_D) s.static_len -= 5u;
  }
  for (int n = heap_len / 2; n >= 1; n--) vsf_pe_downheap(s, heap_len, n);
  int node = elems;
  do {
    const int n = s.heap[1];
    s.heap[1] = s.heap[heap_len--];
    vsf_pe_downheap(s, heap_len, 1);
    const int m = s.heap[1];
    s.heap[--heap_max] = (uint16_t)n;
    s.heap[--heap_max] = (uint16_t)m;
    s.freq[node] = (uint16_t)(s.freq[n] + s.freq[m]);
    s.depth[node] = (uint8_t)((s.depth[n] >= s.depth[m] ? s.depth[n] : s.depth[m]) + 1);
    s.dad[n] = s.dad[m] = (uint16_t)node;
    s.heap[1] = (uint16_t)node++;
    vsf_pe_downheap(s, heap_len, 1);
  } while (heap_len >= 2);
  s.heap[--heap_max] = s.heap[1];
  // gen_bitlen
  for (int b = 0; b <= 15; b++) s.bl_count[b] = 0;
  int overflow = 0, h;
  s.len[s.heap[heap_max]] = 0;
  for (h = heap_max + 1; h < VSF_PE_HEAP; h++) {
    const int n = s.heap[h];
    int bits = s.len[s.dad[n]] + 1;
    if (bits > max_length) {
      bits = max_length;
      overflow++;
    }
    s.len[n] = (uint16_t)bits;
    if (n > max_code) continue;
    s.bl_count[bits]++;
    const int xbits = vsf_pe_extra_bits(which, n);
    const uint32_t f = s.freq[n];
    s.opt_len += f * (uint32_t)(bits + xbits);
    if (which == VSF_PE_TREE_L) s.static_len += f * (uint32_t)(vsf_pe_static_llen(n) + xbits);
    if (which == VSF_PE_TREE_D) s.static_len += f * (uint32_t)(5 + xbits);
  }
  if (overflow > 0) {
    do {
      int bits = max_length - 1;
      while (s.bl_count[bits] == 0) bits--;
      s.bl_count[bits]--;
      s.bl_count[bits + 1] += 2;
      s.bl_count[max_length]--;
      overflow -= 2;
    } while (overflow > 0);
    for (int bits = max_length; bits != 0; bits--) {
      int n = s.bl_count[bits];
      while (n != 0) {
        const int m = s.heap[--h];
        if (m > max_code) continue;
        if (s.len[m] != (uint16_t)bits) {
          s.opt_len += (uint32_t)(bits - (int)s.len[m]) * (uint32_t)s.freq[m];
          s.len[m] = (uint16_t)bits;
        }
        n--;
      }
    }
  }
  // gen_codes
  uint32_t next_code[16], c = 0;
  next_code[0] = 0;
  for (int bits = 1; bits <= 15; bits++) {
    c = (c + s.bl_count[bits - 1]) << 1;
    next_code[bits] = c & 0xFFFFu;
  }
  for (int n = 0; n <= max_code; n++) {
    const int len = s.len[n];
    if (len == 0) continue;
    code[n] = (uint16_t)vsf_pe_reverse(next_code[len]++, len);
  }
  return max_code;
}

// scan_tree (count = true: tally into s.blfreq) and send_tree (count = false: write through `put`) share their walk.
template <typename Put>
VSF_PE_HD void vsf_pe_walk_tree(VsfPeWork& s, const uint16_t* len, int max_code, bool count, Put& put) {
  int prevlen = -1, nextlen = len[0], n_rep = 0, max_count = 7, min_count = 4;
  if (nextlen == 0) {
    max_count = 138;
    min_count = 3;
  }
  for (int n = 0; n <= max_code; n++) {
    const int curlen = nextlen;
    nextlen = len[n + 1];  // (len[max_code + 1] is the guard 0xffff)
    if (++n_rep < max_count && curlen == nextlen) continue;
    if (n_rep < min_count) {
      if (count) {
        s.blfreq[curlen] += (uint16_t)n_rep;
      } else {
        do {
          put(s.blcode[curlen], s.bllen[curlen]);
        } while (--n_rep != 0);
      }
    } else if (curlen != 0) {
      if (curlen != prevlen) {
        if (count)
          s.blfreq[curlen]++;
        else
          put(s.blcode[curlen], s.bllen[curlen]);
        n_rep--;
      }
      if (count) {
        s.blfreq[16]++;
      } else {
        put(s.blcode[16], s.bllen[16]);
        put((uint32_t)(n_rep - 3), 2);
      }
    } else if (n_rep <= 10) {
      if (count) {
        s.blfreq[17]++;
      } else {
        put(s.blcode[17], s.bllen[17]);
        put((uint32_t)(n_rep - 3), 3);
      }
    } else {
      if (count) {
        s.blfreq[18]++;
      } else {
        put(s.blcode[18], s.bllen[18]);
        put((uint32_t)(n_rep - 11), 7);
      }
    }
    n_rep = 0;
    prevlen = curlen;
    if (nextlen == 0) {
      max_count = 138;
      min_count = 3;
    } else if (curlen == nextlen) {
      max_count = 6;
      min_count = 3;
    } else {
      max_count = 7;
      min_count = 4;
    }
  }
}

struct VsfPeHdrWriter {
  uint32_t* words;
  uint32_t bits;
  VSF_PE_HD void operator()(uint32_t value, int len) {
    const uint32_t w = bits >> 5, sh = bits & 31u;
    words[w] |= value << sh;
    if (sh + (uint32_t)len > 32u) words[w + 1] |= value >> (32u - sh);
    bits += (uint32_t)len;
  }
};

VSF_PE_HD int vsf_pe_bl_order(int i) {
  constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return order[i];
}

// _tr_flush_block for a block of `stored_len` bytes whose literal/length frequencies (END_BLOCK included) the caller has put into
// s.freq[0 .. 286) and that holds n_matches matches (all of distance 1: distance code 0).  zlib cannot store a block whose
// start has left its window, and no window is modelled here, because the stored form never wins for such a block:
//   - the start leaves the window only when the block is longer than 32768 - 262 = 32506 bytes;
//   - a block of L literals and M matches has L + M <= 16383; with the static codes it takes at most 9 L + 18 M + 10 bits (a
//     literal 8 or 9 bits; a match 8 + 5 extra + 5 distance at most; END_BLOCK and the header), and it covers B >= L + 3 M bytes,
//     exactly B = L + (sum of the match lengths);
//   - stored wins only if 8 (B + 4) <= bits + 10, so 8 B <= 9 L + 18 M.  With B >= L + 3 M that needs L >= 6 M: M <= 16383 / 7
//     = 2340, and then B <= (9 L + 18 M) / 8 <= (9 * 16383 + 9 * 2340) / 8 < 21100 bytes, under 32506.
// (The dynamic form only lowers the bits further: opt_lenb is the smaller of the two.)
VSF_PE_HD void vsf_pe_plan_block(VsfPeWork& s, uint32_t n_matches, uint32_t stored_len, bool last, VsfPePlan* plan) {
  s.opt_len = s.static_len = 0;
  s.l_max = vsf_pe_build_tree(s, VSF_PE_TREE_L, s.lcode);
  for (int n = 0; n < VSF_PE_L_CODES; n++) s.llen[n] = s.len[n];
  for (int n = 0; n < VSF_PE_D_CODES; n++) s.freq[n] = 0;
  s.freq[0] = (uint16_t)n_matches;
  s.d_max = vsf_pe_build_tree(s, VSF_PE_TREE_D, s.dcode);
  for (int n = 0; n < VSF_PE_D_CODES; n++) s.dlen[n] = s.len[n];
  // build_bl_tree
  for (int n = 0; n < VSF_PE_BL_CODES; n++) s.blfreq[n] = 0;
  s.llen[s.l_max + 1] = 0xFFFF;
  s.dlen[s.d_max + 1] = 0xFFFF;
  VsfPeHdrWriter none{nullptr, 0};
  vsf_pe_walk_tree(s, s.llen, s.l_max, true, none);
  vsf_pe_walk_tree(s, s.dlen, s.d_max, true, none);
  for (int n = 0; n < VSF_PE_BL_CODES; n++) s.freq[n] = s.blfreq[n];
  vsf_pe_build_tree(s, VSF_PE_TREE_BL, s.blcode);
  for (int n = 0; n < VSF_PE_BL_CODES; n++) s.bllen[n] = s.len[n];
  int max_blindex = VSF_PE_BL_CODES - 1;
  for (; max_blindex >= 3; max_blindex--)
    if (s.bllen[vsf_pe_bl_order(max_blindex)] != 0) break;
  s.opt_len += 3u * ((uint32_t)max_blindex + 1u) + 5 + 5 + 4;
  s.max_blindex = max_blindex;
  uint32_t opt_lenb = (s.opt_len + 3 + 7) >> 3;
  const uint32_t static_lenb = (s.static_len + 3 + 7) >> 3;
  if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
  for (int i = 0; i < VSF_PE_HDR_WORDS; i++) plan->hdr[i] = 0;
  VsfPeHdrWriter put{plan->hdr, 0};
  plan->pad_ = 0;
  if (stored_len + 4 <= opt_lenb) {
    plan->type = 0;
    put(last ? 1u : 0u, 3);
    plan->body_bits = 32u + 8u * stored_len;
  } else if (static_lenb == opt_lenb) {
    plan->type = 1;
    put(2u + (last ? 1u : 0u), 3);
    plan->body_bits = s.static_len;
    for (int n = 0; n < VSF_PE_L_CODES; n++) plan->lcode[n] = vsf_pe_static_lcode(n) | (uint32_t)vsf_pe_static_llen(n) << 16;
    plan->dcode0 = 5u << 16;
  } else {
    plan->type = 2;
    put(4u + (last ? 1u : 0u), 3);
    put((uint32_t)(s.l_max + 1 - 257), 5);
    put((uint32_t)(s.d_max + 1 - 1), 5);
    put((uint32_t)(max_blindex + 1 - 4), 4);
    for (int rank = 0; rank <= max_blindex; rank++) put(s.bllen[vsf_pe_bl_order(rank)], 3);
    vsf_pe_walk_tree(s, s.llen, s.l_max, false, put);
    vsf_pe_walk_tree(s, s.dlen, s.d_max, false, put);
    plan->body_bits = s.opt_len - (put.bits - 3u);
    for (int n = 0; n < VSF_PE_L_CODES; n++)
      plan->lcode[n] = n <= s.l_max && s.llen[n] != 0 ? (uint32_t)s.lcode[n] | (uint32_t)s.llen[n] << 16 : 0u;
    plan->dcode0 = (uint32_t)s.dcode[0] | (uint32_t)s.dlen[0] << 16;
  }
  plan->hdr_bits = put.bits;
}

// One symbol (0 .. 255 a literal, 256 + (length - 3) a match, 512 END_BLOCK) as the bits the block's codes give it -> their count.
VSF_PE_HD int vsf_pe_symbol_bits(const uint32_t* lcode, uint32_t dcode0, uint32_t sym, uint64_t* bits) {
  if (sym < 256u || sym == 512u) {
    const uint32_t c = lcode[sym == 512u ? 256 : sym];
    *bits = c & 0xFFFFu;
    return (int)(c >> 16);
  }
  int extra;
  uint32_t value;
  const int lc = vsf_pe_length_code(sym - 256u, &extra, &value);
  const uint32_t c = lcode[257 + lc];
  int n = (int)(c >> 16);
  uint64_t b = c & 0xFFFFu;
  b |= (uint64_t)value << n;
  n += extra;
  b |= (uint64_t)(dcode0 & 0xFFFFu) << n;
  n += (int)(dcode0 >> 16);
  *bits = b;
  return n;  // <= 15 + 5 + 15
}

#endif  // VSF_PNG_ENC_TREES_H_
