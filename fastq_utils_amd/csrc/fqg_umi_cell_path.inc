    // fqg_umi_cell_path.inc - body of fqg_umi_count's cell_path lambda (CR-sorted input, unit increments):
    // counting by one workgroup per cell (fqg_umi_cell_kernels.hip), then the RL_Tree replay on (cell, feature)
    // runs (fqg_umi_rl_kernels.hip, by_cell), with the pair arrays laid out per cell.
    const uint64_t slots = n;  // pair slots: the pairs of a cell start at its first record's index
    Pt.t.s = S.get<KeySlot>(slots);
    Pt.t.mask = 0;
    Pt.reads = S.get<uint32_t>(slots);
    Pt.umis = S.get<uint32_t>(slots);
    uint32_t* d_pair_mem = S.get<uint32_t>(slots);
    uint32_t* d_pair_pos = S.get<uint32_t>(slots);
    uint32_t* d_members = S.get<uint32_t>(slots);
    uint32_t* d_slot_hit = S.get<uint32_t>(slots, 0xFF);
    uint32_t* d_flagged_slot = S.get<uint32_t>(slots);
    uint32_t* d_run_of_slot = S.get<uint32_t>(slots);
    d_new = S.get<uint8_t>(n);
    d_cell_reads = S.get<uint32_t>(n_cells + 2, 0);
    d_cell_umis = S.get<uint32_t>(n_cells + 2, 0);
    d_cell_pairs = S.get<uint32_t>(n_cells + 2, 0);
    d_cloc = S.get<unsigned long long>(n_cells + 2);
    d_cspan = S.get<unsigned long long>(nbc);
    RlCall* d_rl = S.get<RlCall>(1, 0);
    UMI_NEED(Pt.t.s && Pt.reads && Pt.umis && d_pair_mem && d_pair_pos && d_members && d_slot_hit && d_flagged_slot &&
             d_run_of_slot && d_new && d_cell_reads && d_cell_umis && d_cell_pairs && d_cloc && d_cspan && d_rl);
    CellArgs CA;
    memset(&CA, 0, sizeof(CA));
    CA.n = n;
    CA.n_cells = (uint32_t)n_cells;
    CA.feat = ids.feat;
    CA.umi = ids.umi;
    CA.cell_first = d_cell_first;
    CA.is_new = d_new;
    CA.pair_key = Pt.t.s;
    CA.pair_reads = Pt.reads;
    CA.pair_umis = Pt.umis;
    CA.pair_mem = d_pair_mem;
    CA.pair_pos = d_pair_pos;
    CA.members = d_members;
    CA.cell_pairs = d_cell_pairs;
    CA.cell_reads = d_cell_reads;
    CA.cell_umis = d_cell_umis;
    CA.slot_hit = d_slot_hit;
    CA.flagged_slot = d_flagged_slot;
    CA.rl = d_rl;
    CA.call = d_call;
    // LDS keys: the smallest power of two that holds the largest cell, up to 8192 (64 KiB); larger cells sort in memory
    uint32_t lds_keys = 64;
    while (lds_keys < h_call.max_cell_records && lds_keys < 8192u) lds_keys <<= 1;
    CA.lds_keys = lds_keys;
    if (h_call.max_cell_records > lds_keys) {
      CA.big_keys = S.get<unsigned long long>(2ull * n + 128);
      UMI_NEED(CA.big_keys);
    }
    if (lds_keys * 8u > 48u * 1024u) {
      const int rcl = raise_dynamic_lds(c, reinterpret_cast<const void*>(k_umi_cells), (size_t)lds_keys * 8u);
      if (rcl) return rcl;
    }
    {
      ProfScope ps(c, "k_umi_cells");
      hipLaunchKernelGGL(k_umi_cells, dim3((unsigned)n_cells), dim3(kBlock), (size_t)lds_keys * 8u, st, CA);
    }
    // pairs grouped by cell (they already are: a prefix over the cells' pair counts gives the compact order)
    {
      ProfScope ps(c, "k_umi_pairs");
      scan64(c, d_cell_pairs, d_cloc, d_cspan, d_tot + 3, n_cells + 2);
    }
    RlCall h_rl;
    HIP_TRY(c, hipMemcpyAsync(h_tot, d_tot, sizeof(h_tot), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&h_rl, d_rl, sizeof(h_rl), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    n_pairs = h_tot[3];
    const Prefix cst{d_cloc, d_cspan};
    d_pair_of = S.get<uint32_t>(n_pairs);
    UMI_NEED(d_pair_of);
    if (n_pairs) {
      ProfScope ps(c, "k_umi_pairs");
      hipLaunchKernelGGL(k_umi_cell_pairs_fill, dim3((unsigned)n_cells), dim3(kBlock), 0, st, (uint32_t)n_cells,
                         (const uint32_t*)d_cell_first, (const uint32_t*)d_cell_pairs, cst, d_pair_of, d_run_of_slot);
    }
    // ---- the reference's UMI container where it is not a set ----
    const uint32_t n_flagged = prm->strict_set ? 0u : h_rl.n_flagged;
    if (n_flagged) {
      const uint32_t n_runs = (uint32_t)n_pairs;
      RlRuns runs;
      runs.start = S.get<uint32_t>(n_runs);
      runs.len = S.get<uint32_t>(n_runs);
      runs.pslot = d_pair_of;
      runs.flag = S.get<uint32_t>(n_runs, 0xFF);
      uint32_t* d_run_feat = S.get<uint32_t>(n_runs);
      uint32_t* d_run_mem = S.get<uint32_t>(n_runs);
      uint32_t* d_run_nmem = S.get<uint32_t>(n_runs);
      uint32_t* d_flagged = S.get<uint32_t>(n_flagged);
      uint32_t* d_fk0 = S.get<uint32_t>(n_flagged);
      uint32_t* d_flen = S.get<uint32_t>(n_flagged);
      uint32_t* d_foff = S.get<uint32_t>(n_flagged);
      uint32_t* d_fext = S.get<uint32_t>(n_flagged, 0);
      UMI_NEED(runs.start && runs.len && runs.flag && d_run_feat && d_run_mem && d_run_nmem && d_flagged && d_fk0 && d_flen &&
               d_foff && d_fext);
      HIP_TRY(c, hipMemsetAsync(d_rl, 0, sizeof(RlCall), st));
      uint8_t* d_feat_flag = S.get<uint8_t>((uint64_t)n_feat + 2, 0);
      unsigned long long* ck = S.get<unsigned long long>(n_runs);
      unsigned long long* cko = S.get<unsigned long long>(n_runs);
      uint32_t* cv = S.get<uint32_t>(n_runs);
      uint32_t* cvo = S.get<uint32_t>(n_runs);
      uint32_t* pos = S.get<uint32_t>(n_runs);
      UMI_NEED(d_feat_flag && ck && cko && cv && cvo && pos);
      d_feat_replayed = d_feat_flag;
      {
        ProfScope ps(c, "k_rl_detect");
        hipLaunchKernelGGL(k_rl_cell_flags, dim3(blocks_for(n_flagged)), dim3(kBlock), 0, st, n_flagged,
                           (const uint32_t*)d_flagged_slot, (const uint32_t*)d_slot_hit, (const uint32_t*)d_run_of_slot,
                           (const KeySlot*)Pt.t.s, (const uint32_t*)Pt.reads, runs, d_flagged, d_fk0, d_flen, d_feat_flag, d_rl);
        hipLaunchKernelGGL(k_rl_cell_chain, dim3(blocks_for(n_runs)), dim3(kBlock), 0, st, n_runs, (const uint32_t*)d_pair_of,
                           (const KeySlot*)Pt.t.s, (const uint8_t*)d_feat_flag, (const uint32_t*)d_cell_first,
                           (const uint32_t*)d_pair_mem, (const uint32_t*)Pt.umis, runs, d_run_feat, d_run_mem, d_run_nmem, ck, cv,
                           d_rl);
      }
      std::vector<uint32_t> h_len(n_flagged), h_off(n_flagged);
      HIP_TRY(c, hipMemcpyAsync(h_len.data(), d_flen, (size_t)n_flagged * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(&h_rl, d_rl, sizeof(h_rl), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      const uint32_t n_chain = h_rl.n_chain;
      uint32_t cap_nodes = 1u + 8u * h_rl.max_flagged_len + 2048u;
      cap_nodes = (cap_nodes + 63u) & ~63u;
      uint32_t mcap = 64;
      while (mcap < h_rl.max_len) mcap <<= 1;
      uint64_t arena_nodes = 0;
      for (uint32_t f = 0; f < n_flagged; ++f) {
        h_off[f] = (uint32_t)arena_nodes;
        arena_nodes += ((uint64_t)std::min<uint64_t>(cap_nodes, 1ull + 8ull * h_len[f]) + 63u) & ~63ull;
        if (arena_nodes >= 0xFFFFFFFFull) return fail(c, FQG_ERR_STATE, "fqg_umi_count: too many replayed UMI sets");
      }
      uint16_t* d_arena = S.get<uint16_t>(arena_nodes + 64);
      UMI_NEED(d_arena);
      HIP_TRY(c, hipMemcpyAsync(d_foff, h_off.data(), (size_t)n_flagged * 4, hipMemcpyHostToDevice, st));
      RlReplayArgs A;
      memset(&A, 0, sizeof(A));
      {
        ProfScope ps(c, "k_rl_chains");
        uint32_t* ik = S.get<uint32_t>(n_flagged);
        uint32_t* iko = S.get<uint32_t>(n_flagged);
        uint32_t* iv = S.get<uint32_t>(n_flagged);
        uint32_t* ivo = S.get<uint32_t>(n_flagged);
        UMI_NEED(ik && iko && iv && ivo);
        size_t tb = 0, tb2 = 0;
        HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, tb, ck, cko, cv, cvo, (size_t)n_chain, 0, 64, st));
        HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, tb2, ik, iko, iv, ivo, (size_t)n_flagged, 0, 32, st));
        void* tmp2 = S.get<uint8_t>(std::max(tb, tb2) + 16);
        UMI_NEED(tmp2);
        HIP_TRY(c, rocprim::radix_sort_pairs(tmp2, tb, ck, cko, cv, cvo, (size_t)n_chain, 0, 64, st));
        hipLaunchKernelGGL(k_rl_positions, dim3(blocks_for(n_chain)), dim3(kBlock), 0, st, n_chain, (const uint32_t*)cvo, pos);
        hipLaunchKernelGGL(k_rl_item_keys, dim3(blocks_for(n_flagged)), dim3(kBlock), 0, st, n_flagged,
                           (const uint32_t*)d_flagged, (const uint32_t*)pos, ik, iv);
        HIP_TRY(c, rocprim::radix_sort_pairs(tmp2, tb2, ik, iko, iv, ivo, (size_t)n_flagged, 0, 32, st));
        A.chain_runs = cvo;
        A.chain_key = cko;
        A.pos_of_run = pos;
        A.items = ivo;
      }
      A.flagged = d_flagged;
      A.n_items = n_flagged;
      A.runs = runs;
      A.order = nullptr;
      A.umi_id = ids.umi;
      A.cell_id = ids.cell;
      A.is_new = d_new;
      A.flag_k0 = d_fk0;
      A.flag_off = d_foff;
      A.flag_ext = d_fext;
      A.arena = d_arena;
      A.cap = cap_nodes;
      A.mcap = mcap;
      A.by_cell = 1;
      A.rec_feat = ids.feat;
      A.run_feat = d_run_feat;
      A.run_mem = d_run_mem;
      A.run_nmem = d_run_nmem;
      A.members = d_members;
      A.pair_umis = Pt.umis;
      A.cell_umis = d_cell_umis;
      A.n_new_spread = &d_call->spread[2][0];
      A.call = d_rl;
      const uint64_t work_bytes = rl_work_bytes(cap_nodes, mcap);
      const unsigned grid = (unsigned)std::min<uint32_t>(A.n_items, 1024u);
      A.in_lds = work_bytes <= 150u * 1024u;
      if (!A.in_lds) {
        A.scratch_stride = (work_bytes + 255) & ~255ull;
        A.scratch = S.get<uint8_t>(A.scratch_stride * grid);
        UMI_NEED(A.scratch);
      }
      if (A.in_lds && work_bytes > 48u * 1024u) {  // (raised per device and kernel, for the whole process: raise_dynamic_lds)
        const int rcl = raise_dynamic_lds(c, reinterpret_cast<const void*>(k_rl_replay), (size_t)work_bytes);
        if (rcl) return rcl;
      }
      {
        ProfScope ps(c, "k_rl_replay");
        hipLaunchKernelGGL(k_rl_replay, dim3(grid), dim3(kWave), A.in_lds ? (size_t)work_bytes : 0, st, A);
      }
      HIP_TRY(c, hipMemcpyAsync(&h_rl, d_rl, sizeof(h_rl), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      HIP_TRY(c, hipGetLastError());
      if (getenv("FQGPU_RL_DEBUG"))
        fprintf(stderr, "[rl/cells] runs %u flagged %u max_len %u max_flagged_len %u overwrites %u lookback_runs %u changed %u "
                "ticks(100MHz): replay %llu (build %llu loop %llu) lookback %llu store %llu; slowest run: %llu ticks, %llu records, %llu inserts; most look-back (waiting included) in one run: %llu ticks\n", n_runs, n_flagged, h_rl.max_len, h_rl.max_flagged_len,
                h_rl.overwrites, h_rl.lookback_runs, h_rl.changed, h_rl.clk_replay, h_rl.clk_build, h_rl.clk_loop, h_rl.clk_lookback, h_rl.clk_store, h_rl.clk_max >> 32, (h_rl.clk_max >> 16) & 0xFFFF, h_rl.clk_max & 0xFFFF, h_rl.clk_max_wait);
      out->rl_changed = h_rl.changed;
      out->rl_undefined = h_rl.undefined;
      out->rl_unresolved = h_rl.overflow ? 1 : 0;
    }
    out->rl_replayed = n_flagged;
    // ---- float32 counters: unit increments -> the counts as floats (saturating like repeated += 1.0f) ----
    d_pair_reads = S.get<float>(slots);
    d_pair_umis = S.get<float>(slots);
    d_cellf_reads = S.get<float>(n_cells + 2, 0);
    d_cellf_umis = S.get<float>(n_cells + 2, 0);
    UMI_NEED(d_pair_reads && d_pair_umis && d_cellf_reads && d_cellf_umis);
    {
      ProfScope ps(c, "k_umi_sums");
      hipLaunchKernelGGL(k_umi_cell_unit_sums, dim3((unsigned)n_cells), dim3(kBlock), 0, st, (uint32_t)n_cells,
                         (const uint32_t*)d_cell_first, (const uint32_t*)d_cell_pairs, (const uint32_t*)Pt.reads,
                         (const uint32_t*)Pt.umis, d_pair_reads, d_pair_umis);
      hipLaunchKernelGGL(k_umi_unit_sums, dim3(blocks_for(n_cells + 1)), dim3(kBlock), 0, st, n_cells + 1,
                         (const uint32_t*)d_cell_reads, (const uint32_t*)d_cell_umis, d_cellf_reads, d_cellf_umis);
    }
