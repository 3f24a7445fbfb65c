"""How the fp16-operand library (libjat_hip_fp16.so, JAT_OPERAND_DTYPE=fp16) covers every tests/test_gpu_*.py file.  The operand
dtype is chosen once per process, so this process (bf16) never runs that library: a file is covered only where some test starts a
child process for it.  One entry per file, of one of these kinds:

    ("child", [pytest args, ...])    selections of the file that tests/test_gpu_fp16.py runs, each in a child process of its own, on
                                     the fp16 library: the same tests, the same gates.  [] selects the whole file.
    ("same_bits", "test_name")       the file's kernels are compiled into both libraries but do not follow the operand dtype; its
                                     own test `test_name` starts an fp16 child and proves that both libraries give identical bits.
    ("own_child", "test_name")       the file's own test `test_name` starts a child that runs a selection of the file on the fp16
                                     library against the file's gates (not repeated by tests/test_gpu_fp16.py).
    ("independent", "reason")        nothing in the file launches a kernel that no other entry covers on fp16, or it is
                                     tests/test_gpu_fp16.py itself.

tests/test_fp16_matrix_cpu.py keeps the table complete: a new tests/test_gpu_*.py fails the CPU suite until it has an entry.

A `-k` word matches as a substring of the test id AND of the file's name, so no word below is part of its file's name ("ema" would
select all of test_gpu_ema.py)."""

MATRIX = {
    "test_gpu_kernels.py": ("child", [[]]),
    "test_gpu_train_kernels.py": ("child", [[]]),
    "test_gpu_model.py": ("child", [["-k", "forward_vs_reference or sampler_vs_reference or benchmarked or fused"]]),
    # every launch path at full width, gated on the fp16 rounding floor
    "test_gpu_forward_paths.py": ("child", [[]]),
    "test_gpu_widths.py": ("child", [
        # the other hidden sizes: norm_modulate_kernel and linear_f32_kernel's SiLU output store through jat_dtype.h
        ["-k", "norm or time_embed or forward"],
        # two sampler steps (default, default-folded, forced folding) and the training step at 768 / 1024 / 1536 / 2048; the
        # three switch children, which start grandchildren, stay out
        ["-k", "two_sampler_steps or train_step_at_width"]]),
    "test_gpu_train.py": ("child", [
        ["-k", "train_step_vs_reference_golden or v3mod2 or scale_invariant or non_finite or skipped_step or fp16"]]),
    # EPI_CFG_EULER: ce_patch is stored through jat_dtype.h.  The sampler cases at micro only (wide2 adds run time, not coverage)
    "test_gpu_sampler_tail.py": ("child", [
        ["-k", "kernel_fused_tail or kernel_rejects or (sampler_fused_tail and micro)"]]),
    # EPI_CFG_STAGE, cfg_stage_kernel, midpoint and Heun
    "test_gpu_solvers.py": ("child", [
        ["-k", "kernel_fused_stage or cfg_stage_step or sampler_against_the_fp64_twin or midpoint_on_the_unfused or "
               "(fused_stage_tail and micro) or short_row_under_midpoint"]]),
    # the ACC instantiations of gemm_tn.hip / train.hip, the 1 / k un-scale factor, the skipped step; without the single-rank RCCL
    # test, the fit tests and wide2 at T = 1378
    "test_gpu_grad_accum.py": ("child", [
        ["-k", "weight_grad_accumulate or (three_accumulated and not wide2) or vs_numpy_oracle or k_equal_micro or "
               "non_finite_micro or miscounted or real_overflow"]]),
    # adamw_ema_kernel under the trainer; the kernel test at its two smaller n; without checkpoints and fit
    "test_gpu_ema.py": ("child", [
        ["-k", "(fused_adamw and not 1000004) or non_finite_gradient or swap_exchanges or follows_the_fp64 or weights_context or "
               "across_real"]]),
    # every side-stream case: the whole file takes 18 s on the MI355X, less than the other children
    "test_gpu_streams.py": ("child", [[]]),
    # the four model entries: the only workspaces here whose kernels follow the operand dtype
    "test_gpu_workspaces.py": ("child", [["-k", "model"]]),
    "test_gpu_mod3_train.py": ("own_child", "test_fp16_library_runs_the_mod3_step"),
    # latent_loss_kernel / latent_loss_fft_kernel: fp32 kernels of train.hip, a translation unit compiled with -DJAT_FP16
    "test_gpu_loss_paths.py": ("same_bits", "test_fp16_library_gives_the_same_bits"),
    "test_gpu_mod3_loss.py": ("independent", "the kernels of test_gpu_loss_paths.py, whose test_fp16_library_gives_the_same_bits "
                                             "runs jat_k_latent_loss_ex with recon_eps = 0 and 1e-6 on both libraries"),
    "test_gpu_splice.py": ("same_bits", "test_fp16_library_gives_the_same_bits"),
    "test_gpu_data.py": ("same_bits", "test_fp16_library_gives_the_same_bits"),
    "test_gpu_metrics.py": ("same_bits", "test_fp16_library_gives_the_same_bits"),
    "test_gpu_resample.py": ("same_bits", "test_fp16_library_gives_the_same_bits"),
    "test_gpu_resample_shapes.py": ("independent", "resample_kernel<1>, resample_kernel<4> and the statistics kernels do not follow "
                                                   "the operand dtype; test_fp16_library_gives_the_same_bits of test_gpu_resample.py "
                                                   "runs both instantiations and a sliced conversion on both libraries"),
    "test_gpu_retrieval.py": ("same_bits", "test_fp16_library_gives_the_same_bits"),
    "test_gpu_dac.py": ("same_bits", "test_fp16_library_same_bits"),
    "test_gpu_dac_encoder.py": ("same_bits", "test_fp16_library_same_bits"),
    "test_gpu_fp16.py": ("independent", "the runner of the child entries itself"),
    "test_gpu_fit.py": ("independent", "the fit tool is host code over Trainer, LatentStore and validate: it adds no kernel, and the "
                                       "trainer's step runs on fp16 in the children of test_gpu_train.py, test_gpu_grad_accum.py and "
                                       "test_gpu_ema.py"),
    "test_gpu_infer.py": ("independent", "the inference tool is host code over the sampler and the DAC: it adds no kernel, the "
                                         "sampler runs on fp16 in the children of test_gpu_model.py and test_gpu_solvers.py, and "
                                         "the DAC files prove the same bits"),
    "test_gpu_prepare.py": ("independent", "dataset preparation composes the resampler, the DAC encoder and the statistics kernel, "
                                           "each proved bit-identical in both libraries by its own file; its two inference tests "
                                           "add no kernel to test_gpu_infer.py"),
}

KINDS = ("child", "same_bits", "own_child", "independent")


def children():
    """[(id, [pytest args])] of every child tests/test_gpu_fp16.py runs, in the table's order: `<file stem>` or `<file stem>-<i>`."""
    out = []
    for name, (kind, what) in MATRIX.items():
        if kind != "child":
            continue
        stem = name[len("test_gpu_"):-len(".py")]
        for i, args in enumerate(what):
            out.append((stem if len(what) == 1 else f"{stem}-{i}", ["tests/" + name] + list(args)))
    return out


def k_words(args):
    """The words of the `-k` expression among `args`, without the operators and parentheses."""
    if "-k" not in args:
        return []
    expr = args[args.index("-k") + 1].replace("(", " ").replace(")", " ")
    return [w for w in expr.split() if w not in ("and", "or", "not")]
