#!/usr/bin/env python3
"""Embeds plan.hpp, vm_core.hpp and kernel_body.inc as C++ raw string literals (includes / pragmas stripped) so that
kernels.hip can hand them to hiprtc together with the code generated for one plan.

`embed_sources.py --rw FILE` writes the REVIEW-WORDS variant of the kernel body (review_words.hpp) as kKernelBodyRw: kernel_body.inc itself
stays as it is -- the bytecode build, the kernel emulator and the pinned texts of small tables include it -- and the hooks are the
anchored insertions of RW_HOOKS below, applied here.  An anchor that is missing or matches more than once fails the build.

`embed_sources.py --cold FILE` writes the COLD-ARGS variants (cold_args.hip: launch arguments that one stage reads come from the
kernel-argument segment at the head of that stage) as kKernelBodyCold and, with the review-words hooks applied first, kKernelBodyRwCold:
the sections of cold_args.hip go in at the anchors of cold_hooks() below, under the same rule.  `--cold-body FILE [--rw]` writes one
variant as plain text (what tools/jit_inspect.py --body and GK_JIT_BODY_FILE take); `--cold-struct FILE` writes the parameter struct of
cold_args.hip as code: kernels.hip builds its launch arguments from it."""
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))


def text(name):
    out = []
    for line in open(os.path.join(here, name), encoding="utf-8"):
        if line.startswith("#include") or line.startswith("#pragma once"):
            continue
        out.append(line)
    return "".join(out)


# (anchor, where, inserted text).  where: "inline" = right behind the anchor, inside its line; "before" = whole lines in front of the one
# line that contains the anchor.
RW_HOOKS = [
    # 1. two trailing kernel parameters: rwords[GK_RW_K][rw_stride], the words the binding pass left per review
    ("uint32_t dbg, uint32_t rpp", "inline", ", const uint32_t* __restrict__ rwords, uint32_t rw_stride"),
    # 2. the GK_RW_K words of "my" review in an item, requested by the waves that go on to OR them (one wave per half); same index
    #    arithmetic as flags_of, zero beyond the group's reviews ...
    ("  auto entry_of = [&](const Item& it, uint32_t tid_now) -> ChunkDesc {", "before",
     "  uint32_t rwv[GK_RW_K];\n"
     "  auto rw_of = [&](const Item& it) {\n"
     "    const uint32_t t0 = tile_of(it) * GK_RPT_K, nr = min((uint32_t)GK_RPT_K, n_reviews - t0), g = it.pass * RPP + rl2;\n"
     "    const bool mine = it.ok && wave_on && part == 0u && g < nr;\n"
     "#pragma unroll\n"
     "    for (uint32_t k = 0; k < (uint32_t)GK_RW_K; k++) { const uint32_t* __restrict__ wk = rwords + (size_t)k * rw_stride; rwv[k] = mine ? wk[t0 + g] : 0u; }   // (a scalar base per word, one vector offset for all)\n"
     "  };\n"),
    #    ... at the start of the item's phase 1, behind the clearing barrier: the loads have the chunk loop to land, and no register stays
    #    live across the formulas and the output stage (requested with the next item's flags, as the flags are, measured slower:
    #    profiles/review_words.md)
    ("    const uint2* wl = s_work[buf];", "before", "    rw_of(it);\n"),
    # 3. behind the chunk loop, in front of the barrier that ends phase 1: OR-ed into the review's global words (LDS atomics without
    #    return: other waves may still be OR-ing into the same words)
    ("    GK_PROF(2);", "before",
     "    if (wave_on && part == 0u) {\n"
     "#pragma unroll\n"
     "      for (uint32_t k = 0; k < (uint32_t)GK_RW_K; k++)\n"
     "        (void)__hip_atomic_fetch_or(&lds[GK_RW_WORD(k) * RPP + rl2], rwv[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
     "    }\n"),
]


def sections(name):
    """the `//== name` sections of a stage file"""
    out, cur = {}, None
    for line in open(os.path.join(here, name), encoding="utf-8"):
        if line.startswith("//== "):
            cur = line[5:].strip()
            if cur in out:
                sys.exit("embed_sources.py: section %r twice in %s" % (cur, name))
            out[cur] = ""
        elif cur is not None:
            out[cur] += line
    return out


# where: "replace" = the anchor itself, once in the text; ("until", anchor2) = the lines from the one that contains the anchor up to, not
# including, the one that contains anchor2.
def cold_sections():
    s = sections("cold_args.hip")
    want = {"args", "device", "carried", "tail_head", "tail", "epilogue"}
    if set(s) != want:
        sys.exit("embed_sources.py: cold_args.hip has sections %s, expected %s" % (sorted(s), sorted(want)))
    return s


def cold_hooks():
    s = cold_sections()
    return [
        # 1. the parameter list as a struct and the scalar loads from the argument segment, in front of the kernel
        ("GK_KERNEL_LINKAGE __global__ GK_TILES_BOUNDS void GK_KERNEL_TILES(", "before", s["args"] + s["device"]),
        # 2. the next item's requests take their arrays from two variables that every tail assigns from the segment
        ("  auto flags_of = [&](const Item& it, uint32_t tid_now) -> uint32_t {", "before", s["carried"]),
        ("rflags[t0 + g]", "replace", "rflags_c[t0 + g]"),
        ("lists[(size_t)tile_of(it) * capg + tid_now]", "replace", "lists_c[(size_t)tile_of(it) * capg + tid_now]"),
        # 3. the tail: its arguments requested in front of the flag ballots; the output stage on them
        ("    const unsigned long long ovf_mask = __ballot(ovf);", "before", s["tail_head"]),
        ("    constexpr uint32_t OUT_B = ", ("until", "    GK_PROF(6);"), s["tail"]),
        # 4. the totals row a workgroup leaves with
        ("  __syncthreads();   // every output wave's adds are in", ("until", "#undef GK_MAKE_ACC"), s["epilogue"]),
    ]


def with_hooks(body, hooks):
    for anchor, where, ins in hooks:
        if where == "replace":
            if body.count(anchor) != 1:
                sys.exit("embed_sources.py: anchor %r matches %d times in kernel_body.inc" % (anchor, body.count(anchor)))
            body = body.replace(anchor, ins)
            continue
        if isinstance(where, tuple):
            lines = body.split("\n")
            at = [i for i, line in enumerate(lines) if anchor in line]
            if len(at) != 1:
                sys.exit("embed_sources.py: anchor %r matches %d lines of kernel_body.inc" % (anchor, len(at)))
            to = [i for i, line in enumerate(lines) if where[1] in line]
            if len(to) != 1 or to[0] <= at[0]:
                sys.exit("embed_sources.py: end anchor %r matches %d lines of kernel_body.inc, or none behind %r" % (where[1], len(to), anchor))
            lines[at[0]:to[0]] = ins.rstrip("\n").split("\n")
            body = "\n".join(lines)
            continue
        if where == "inline":
            if body.count(anchor) != 1:
                sys.exit("embed_sources.py: anchor %r matches %d times in kernel_body.inc" % (anchor, body.count(anchor)))
            body = body.replace(anchor, anchor + ins)
            continue
        lines = body.split("\n")
        at = [i for i, line in enumerate(lines) if anchor in line]
        if len(at) != 1:
            sys.exit("embed_sources.py: anchor %r matches %d lines of kernel_body.inc" % (anchor, len(at)))
        new = ins.rstrip("\n").split("\n")
        i = at[0]
        lines[i:i] = new
        body = "\n".join(lines)
    return body


if sys.argv[1] == "--cold":
    with open(sys.argv[2], "w", encoding="utf-8") as f:
        plain = text("kernel_body.inc")
        f.write("static const char kKernelBodyCold[] = R\"GKSRC(%s)GKSRC\";\n" % with_hooks(plain, cold_hooks()))
        f.write("static const char kKernelBodyRwCold[] = R\"GKSRC(%s)GKSRC\";\n" % with_hooks(with_hooks(plain, RW_HOOKS), cold_hooks()))
elif sys.argv[1] == "--cold-struct":
    with open(sys.argv[2], "w", encoding="utf-8") as f:
        f.write(cold_sections()["args"])
elif sys.argv[1] == "--cold-body":
    with open(sys.argv[2], "w", encoding="utf-8") as f:
        plain = text("kernel_body.inc")
        f.write(with_hooks(with_hooks(plain, RW_HOOKS) if "--rw" in sys.argv[3:] else plain, cold_hooks()))
elif sys.argv[1] == "--rw":
    with open(sys.argv[2], "w", encoding="utf-8") as f:
        f.write("static const char kKernelBodyRw[] = R\"GKSRC(%s)GKSRC\";\n" % with_hooks(text("kernel_body.inc"), RW_HOOKS))
else:
    with open(sys.argv[1], "w", encoding="utf-8") as f:
        for var, name in (("kPlanHpp", "plan.hpp"), ("kVmCoreHpp", "vm_core.hpp"), ("kKernelBody", "kernel_body.inc")):
            f.write("static const char %s[] = R\"GKSRC(%s)GKSRC\";\n" % (var, text(name)))
