// sl_gp4_mean.h - what the launcher of the block-mode GP sweep (sl_gp4.hip) needs of
// k_gp_mean_blocks (sl_gp4_mean.hip): one launch per segment of source tiles.
#pragma once
#include "sl_common.h"

struct Gp4MeanLaunch {
    int workgroups;                  // sl_gp4_mean_workgroups(ctx, tiles of the segment)
    long long tile0, tile1;          // source tiles of the segment (of the shard: tile t starts at lo + 64 t)
    sl_key* partials;                // 4 keys per workgroup, one per wavefront
    int fold;                        // a later segment: fold the keys already there
    unsigned long long* ticket;      // tile counter, zeroed by the launcher
    unsigned* list_count;            // records appended, zeroed by the launcher
    long long* list_cell;            // [list_cap] first cell of every open block
    double* list_mean;               // [list_cap][16][d] its posterior means
    unsigned list_cap;
};

int sl_gp4_mean_workgroups(const sl_ctx* ctx, long long tiles);
// development builds (-DSL_DIAG of sl_gp4_mean.hip): blocks decided before panel 0 since the last
// call; 0 otherwise
unsigned long long sl_gp4_mean_decided_fetch(sl_ctx* ctx);

template <int D>
int sl_gp4_mean_launch_dim(sl_ctx* ctx, const SlDevModel& model, const SlSweepArgs& a, const Gp4MeanLaunch& m);
#define SL_GP4_MEAN_DECL(D_)                                                                                 \
    template <> int sl_gp4_mean_launch_dim<D_>(sl_ctx*, const SlDevModel&, const SlSweepArgs&, const Gp4MeanLaunch&);
SL_GP4_MEAN_DECL(1) SL_GP4_MEAN_DECL(2) SL_GP4_MEAN_DECL(3) SL_GP4_MEAN_DECL(4)
#undef SL_GP4_MEAN_DECL
