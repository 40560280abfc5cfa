"""ctypes binding of the database / result-file part of include/starphase_hip.h (sp_database_*, sp_variant_gene_*, sp_result_*,
sp_gene_details_*).  Host only: none of these calls needs a device.  No logic lives here."""
import ctypes as C

import numpy as np

from . import ffi
from .ffi import SP_OK, StarphaseError, sp_hla_db_desc, sp_cyp_locus, sp_cyp_gene_def, sp_cyp_config, sp_variant_problem, sp_sv_definitions

_vp, _u32, _i32, _u64, _i64, _s = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64, C.c_int64, C.c_char_p


class sp_database_metadata(C.Structure):
    _fields_ = [(k, _s) for k in ("pbstarphase_version", "cpic_version", "hla_version", "pharmvar_version", "build_time")]


class sp_database_stats(C.Structure):
    _fields_ = [(k, _u32) for k in ("n_gene_entries", "n_hla_sequences", "n_hla_genes", "n_cyp2d6_alleles", "n_collection_genes")] + \
               [(k, _i32) for k in ("has_hla_config", "has_cyp2d6_config", "reserved")]


class sp_gene_region(C.Structure):
    _fields_ = [("name", _s), ("chrom", _s), ("start", _u64), ("end", _u64), ("is_forward_strand", _i32), ("is_absent_capable", _i32),
                ("n_exons", _u32), ("reserved", _u32), ("exon_start", C.POINTER(_u64)), ("exon_end", C.POINTER(_u64))]


class sp_variant_gene_stats(C.Structure):
    _fields_ = [(k, _u32) for k in ("n_haplotypes", "n_variants", "n_skipped_haplotypes", "n_full_deletions", "n_partial_deletions", "reserved")]


class sp_vcf_allele(C.Structure):
    _fields_ = [("position", _u64), ("ref", _s), ("alt", _s), ("gt", _i32), ("reserved", _i32), ("ps", _i64)]


class sp_vcf_deletion(C.Structure):
    _fields_ = [("start", _u64), ("end", _u64), ("gt", _i32), ("reserved", _i32), ("ps", _i64)]


class sp_variant_detail(C.Structure):
    _fields_ = [("variant_id", _u64), ("variant_name", _s), ("dbsnp", _s), ("chrom", _s), ("position", _u64), ("reference", _s), ("alternate", _s),
                ("sv_label", _s), ("sv_start", _u64), ("sv_end", _u64), ("genotype", _i32), ("is_core_variant", _i32), ("phase_set", _i64)]


class sp_mapping_stats(C.Structure):
    _fields_ = [("present", _i32), ("has_clips", _i32), ("seq_len", _u64), ("nm", _u64), ("unmapped", _u64), ("clipped_start", _u64), ("clipped_end", _u64)]


class sp_detailed_mapping(C.Structure):
    _fields_ = [("present", _i32), ("reserved", _i32), ("query_len", _u64), ("target_len", _u64), ("match_len", _u64), ("nm", _u64),
                ("query_unmapped", _u64), ("target_unmapped", _u64), ("cigar", _s), ("md", _s)]


class sp_diplotype_settings(C.Structure):
    _fields_ = [(k, _s) for k in ("include_set", "exclude_set", "sample_name", "sv_vcf", "debug_folder")] + [("max_sv_length", _u64)] + \
               [("disable_cdna_scoring", _i32), ("hla_require_dna", _i32)] + [(k, C.c_double) for k in ("max_error_rate", "min_cdf_prob", "expected_maf")] + \
               [("infer_connections", _i32), ("normalize_d6_only", _i32), ("min_consensus_fraction", C.c_double),
                ("min_consensus_count", _u64), ("dual_max_ed_delta", _u64), ("debug_skip_hla", _i32), ("sequential", _i32)]


class sp_sample_inputs(C.Structure):
    _fields_ = [("n_bams", _u32), ("bams", C.POINTER(_s)), ("vcf", _s), ("sv_vcf", _s), ("sample_name", _s)]


class sp_cyp_read_mapping(C.Structure):
    _fields_ = [("read", _u32), ("consensus", _u32), ("read_start", _u64), ("read_end", _u64), ("index_label", C.c_char * 64)]


class sp_starphase_timing(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("call_ms", "bam_decode_ms", "variant_ms", "hla_ms", "cyp_ms")] + [("n_hla_reads", _u32), ("n_cyp_reads", _u32)]


class sp_batch_options(C.Structure):
    _fields_ = [("max_group", _u32), ("decode_threads", _u32), ("reserved_", _u32 * 6)]


class sp_starphase_batch_timing(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("wall_ms", "decode_ms", "variant_ms", "hla_ms", "cyp_ms", "package_ms")] + \
               [(k, _u32) for k in ("n_samples", "n_groups", "n_failed", "reserved_")] + [("n_hla_reads", _u64), ("n_cyp_reads", _u64)]


class sp_hla_alleles_stats(C.Structure):
    _fields_ = [(k, _u32) for k in ("n_alleles", "n_dna", "n_dropped_no_cdna", "n_dropped_gene")] + [("warnings", _s)]


class sp_hla_cfg_mapping(C.Structure):
    _fields_ = [(k, _i32) for k in ("status", "rev", "nm", "q_start", "q_end", "t_start", "t_end", "gene")]


class sp_hla_cfg_gene(C.Structure):
    _fields_ = [("name", _s), ("chrom", _s), ("start", _u64), ("end", _u64), ("moved", _i32), ("is_absent_capable", _i32), ("worst_allele", _i32),
                ("worst_len", _i32), ("worst_nm", _i32), ("worst_unmapped", _i32), ("n_dna_alleles", _u32), ("n_mapped", _u32)]


SUBALLELE_MATCH, CORE_MATCH, INEXACT_DIPLOTYPES, FROM_MAPPINGS, FROM_MULTI_MAPPINGS, NO_MATCH = range(6)
_bound = False


def _lib():
    global _bound
    L = ffi.lib()
    if _bound:
        return L
    P = C.POINTER
    sigs = {
        "sp_database_load": (_i32, [_s, P(_vp), _s, _u32]),
        "sp_database_parse": (_i32, [_s, _u64, P(_vp), _s, _u32]),
        "sp_database_free": (None, [_vp]),
        "sp_database_last_error": (_s, [_vp]),
        "sp_database_get_metadata": (_i32, [_vp, P(sp_database_metadata)]),
        "sp_database_info": (_i32, [_vp, P(sp_database_stats)]),
        "sp_database_hla_gene": (_i32, [_vp, _u32, P(sp_gene_region)]),
        "sp_database_gene_entry": (_i32, [_vp, _u32, P(_s), P(_s)]),
        "sp_database_hla_flatten": (_i32, [_vp, _u32, P(_s), P(_s), _i32, P(sp_hla_db_desc)]),
        "sp_database_hla_allele": (_i32, [_vp, _u32, P(_s), P(_s), P(_s)]),
        "sp_database_cyp_window": (_i32, [_vp, P(_s), P(_u64), P(_u64)]),
        "sp_database_cyp_flatten": (_i32, [_vp, _s, _u64, _u64, P(sp_cyp_locus), P(sp_cyp_gene_def), P(sp_cyp_config)]),
        "sp_variant_gene_create": (_i32, [_vp, _s, _s, _u64, P(_vp)]),
        "sp_variant_gene_free": (None, [_vp]),
        "sp_variant_gene_info": (_i32, [_vp, P(sp_variant_gene_stats)]),
        "sp_variant_gene_haplotype": (_i32, [_vp, _u32, P(_s), P(_s)]),
        "sp_variant_gene_variant": (_i32, [_vp, _u32, P(_u64), P(_s), P(_s), P(_s), P(_s), P(_i64), P(_i32)]),
        "sp_variant_gene_sv_definitions": (_i32, [_vp, P(sp_sv_definitions)]),
        "sp_variant_gene_sv_label": (_i32, [_vp, _i32, _i32, P(_s)]),
        "sp_variant_gene_problem": (_i32, [_vp, _u32, P(sp_vcf_allele), _u32, P(sp_vcf_deletion), _u64, P(sp_variant_problem)]),
        "sp_variant_gene_problem_variant": (_i32, [_vp, _i32, P(_i32), P(_s), P(_u64), P(_u64)]),
        "sp_variant_gene_problem_sv_label": (_i32, [_vp, _i32, P(_s)]),
        "sp_variant_gene_last_error": (_s, [_vp]),
        "sp_result_create": (_i32, [_vp, _s, P(_vp)]),
        "sp_result_free": (None, [_vp]),
        "sp_result_last_error": (_s, [_vp]),
        "sp_gene_details_create": (_i32, [P(_vp)]),
        "sp_gene_details_free": (None, [_vp]),
        "sp_gene_details_add_diplotype": (_i32, [_vp, _s, _s]),
        "sp_gene_details_add_simple_diplotype": (_i32, [_vp, _s, _s]),
        "sp_gene_details_set_simple_diplotypes": (_i32, [_vp, _i32]),
        "sp_gene_details_add_inexact_diplotype": (_i32, [_vp, _s, _u32, P(_s), _vp, _vp, _s, _u32, P(_s), _vp, _vp]),
        "sp_gene_details_add_diplotype_only": (_i32, [_vp, _s, _s]),
        "sp_gene_details_add_variant": (_i32, [_vp, P(sp_variant_detail)]),
        "sp_gene_details_add_mapping": (_i32, [_vp, _s, _s, _s, P(sp_mapping_stats), P(sp_mapping_stats), _i32]),
        "sp_gene_details_add_multi_mapping": (_i32, [_vp, _s, _u64, _u64, _u64, _s]),
        "sp_result_insert": (_i32, [_vp, _s, _vp, _i32]),
        "sp_result_json": (_i32, [_vp, P(_s), P(_u64)]),
        "sp_result_save": (_i32, [_vp, _s]),
        "sp_result_pharmcat_tsv": (_i32, [_vp, P(_s), P(_u64)]),
        "sp_result_save_pharmcat_tsv": (_i32, [_vp, _s]),
        "sp_aln_strings": (_i32, [P(ffi.sp_aln), _vp, _s, _u64, _s, _u32, _s, _u32, P(_u64)]),
        "sp_affine_cigar_strings": (_i32, [_vp, _vp, _u32, _s, _u64, _s, _u32, _s, _u32, P(_u64)]),
        "sp_affine_cigar_strings_eqx": (_i32, [_vp, _vp, _u32, _s, _u64, _s, _u32, _s, _u32, P(_u64)]),
        "sp_hla_debug_create": (_i32, [P(_vp)]),
        "sp_hla_debug_free": (None, [_vp]),
        "sp_hla_debug_last_error": (_s, [_vp]),
        "sp_hla_debug_add_read": (_i32, [_vp, _s, _s, _s, _s]),
        "sp_hla_debug_add_mapping": (_i32, [_vp, _s, _s, _s, P(sp_detailed_mapping), P(sp_detailed_mapping)]),
        "sp_hla_debug_add_dual_stats": (_i32, [_vp, _s, P(ffi.sp_hla_call)]),
        "sp_hla_debug_json": (_i32, [_vp, P(_s), P(_u64)]),
        "sp_hla_debug_save": (_i32, [_vp, _s]),
        "sp_cyp_diplotype_mappings": (_i32, [_vp, P(ffi.sp_cyp_problem), _vp, P(ffi.sp_cyp_call), _s, _u32, P(ffi.sp_cyp_region_variants), P(sp_cyp_read_mapping),
                                             _u64, P(_u64)]),
        "sp_cyp_consensus_support": (_i32, [_vp, _vp, P(ffi.sp_cyp_call), _vp, _u32, P(sp_cyp_read_mapping), _u64, _vp, _vp, _u64, _vp]),
        "sp_cyp_consensus_support_cohort": (_i32, [_vp, _u32, P(_vp), P(ffi.sp_cyp_call), _vp, _u32, P(sp_cyp_read_mapping), _vp, _vp, _vp, _u64, _vp]),
        "sp_cyp_support_json": (_i32, [P(ffi.sp_cyp_call), _vp, _u32, _vp, _vp, _vp, _s, _u64, P(_u64)]),
        "sp_cyp_consensus_support_ins": (_i32, [_vp, _vp, P(ffi.sp_cyp_call), _vp, _u32, P(sp_cyp_read_mapping), _u64, _vp, _vp, _u64, _vp, _vp, _u64, P(_u64)]),
        "sp_cyp_consensus_support_cohort_ins": (_i32, [_vp, _u32, P(_vp), P(ffi.sp_cyp_call), _vp, _u32, P(sp_cyp_read_mapping), _vp, _vp, _vp, _u64, _vp, _vp, _u64, P(_u64)]),
        "sp_cyp_support_json_ins": (_i32, [P(ffi.sp_cyp_call), _vp, _u32, _vp, _vp, _vp, _vp, _u64, P(sp_cyp_read_mapping), _u64, P(C.c_char_p), _u32, _s, _u64, P(_u64)]),
        "sp_cyp_consensus_support_hap": (_i32, [_vp, _vp, P(ffi.sp_cyp_call), _vp, _u32, P(sp_cyp_read_mapping), _u64, _vp, _vp, _u64, _vp, _vp, _u64, P(_u64), _vp, _u64, P(_u64), _vp]),
        "sp_cyp_consensus_support_cohort_hap": (_i32, [_vp, _u32, _vp, _vp, _vp, _u32, P(sp_cyp_read_mapping), _vp, _vp, _vp, _u64, _vp, _vp, _u64, P(_u64), _vp, _u64, P(_u64), _vp]),
        "sp_cyp_support_json_hap": (_i32, [P(ffi.sp_cyp_call), _vp, _u32, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, P(sp_cyp_read_mapping), _u64, P(C.c_char_p), _u32, _s, _u64, P(_u64)]),
        "sp_cyp_variant_windows": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, _u32, _vp, _vp]),
        "sp_cyp_variant_support": (_i32, [_vp, P(ffi.sp_cyp_problem), _vp, P(ffi.sp_cyp_call), _vp, _u32, P(ffi.sp_cyp_region_variants), P(sp_cyp_read_mapping), _u64, _u32,
                                          _vp, _vp, _vp, _vp, _u64, _vp]),
        "sp_cyp_variant_support_cohort": (_i32, [_vp, P(ffi.sp_cyp_problem), _u32, _vp, _vp, _vp, _u32, _vp, P(sp_cyp_read_mapping), _vp, _u32, _vp, _vp, _vp, _vp, _u64, _vp]),
        "sp_cyp_alleles_vcf": (_i32, [_vp, P(ffi.sp_cyp_call), P(ffi.sp_cyp_region_variants), _vp, _vp, _s, _s, _vp, _u64, P(_u64)]),
        "sp_cyp_alleles_vcf_save": (_i32, [_vp, P(ffi.sp_cyp_call), P(ffi.sp_cyp_region_variants), _vp, _vp, _s, _s, _s]),
        "sp_bgzf_save": (_i32, [_s, _vp, _u64]),
        "sp_starphase_set_cyp_vcf": (_i32, [_vp, _i32]),
        "sp_starphase_set_cyp_alternatives": (_i32, [_vp, _i32]),
        "sp_starphase_set_cyp_alternative_reads": (_i32, [_vp, _i32]),
        "sp_starphase_set_variant_alternatives": (_i32, [_vp, _i32]),
        "sp_diplotype_settings_default": (None, [P(sp_diplotype_settings)]),
        "sp_diplotype_settings_check": (_i32, [P(sp_diplotype_settings), P(sp_sample_inputs), _s, _u32]),
        "sp_starphase_create": (_i32, [_vp, _s, _s, P(sp_diplotype_settings), P(_vp)]),
        "sp_starphase_free": (None, [_vp]),
        "sp_starphase_last_error": (_s, [_vp]),
        "sp_starphase_call": (_i32, [_vp, P(sp_sample_inputs), P(_vp)]),
        "sp_starphase_warnings": (_s, [_vp]),
        "sp_starphase_last_timing": (_i32, [_vp, P(sp_starphase_timing)]),
        "sp_starphase_set_read_debug": (_i32, [_vp, _i32]),
        "sp_starphase_set_hla_debug_mappings": (_i32, [_vp, _i32]),
        "sp_starphase_set_hla_ties": (_i32, [_vp, _i32]),
        "sp_starphase_set_consensus_support": (_i32, [_vp, _i32]),
        "sp_starphase_set_cyp_consensus_support": (_i32, [_vp, _i32]),
        "sp_starphase_set_support_insertions": (_i32, [_vp, _i32]),
        "sp_starphase_set_support_haplotypes": (_i32, [_vp, _i32]),
        "sp_starphase_call_batch": (_i32, [_vp, _u32, P(sp_sample_inputs), P(_s), P(sp_batch_options), P(_vp), P(_i32)]),
        "sp_starphase_sample_error": (_s, [_vp, _u32]),
        "sp_starphase_sample_warnings": (_s, [_vp, _u32]),
        "sp_starphase_last_batch_timing": (_i32, [_vp, P(sp_starphase_batch_timing)]),
        "sp_cyp_diplotype_cohort_mappings": (_i32, [_vp, P(ffi.sp_cyp_problem), _u32, P(_vp), P(ffi.sp_cyp_call), _s, _u32, P(ffi.sp_cyp_region_variants),
                                                    P(sp_cyp_read_mapping), _u64, P(_u64), P(_i32)]),
        "sp_hla_fasta_load": (_i32, [_s, _s, P(_vp)]),
        "sp_hla_fasta_last_error": (_s, []),
        "sp_hla_alleles_free": (None, [_vp]),
        "sp_hla_alleles_info": (_i32, [_vp, P(sp_hla_alleles_stats)]),
        "sp_hla_alleles_get": (_i32, [_vp, _u32, P(_s), P(_s), P(_s), P(_s), P(_s)]),
        "sp_hla_config_extend": (_i32, [_vp, _vp, _vp, _vp, _u32, P(_vp)]),
        "sp_hla_config_result_create": (_i32, [_u32, P(_s), P(_u64), P(_u64), P(_vp)]),
        "sp_hla_config_result_free": (None, [_vp]),
        "sp_hla_config_result_info": (_i32, [_vp, P(_u32), P(_u32), P(_s)]),
        "sp_hla_config_result_gene": (_i32, [_vp, _u32, P(sp_hla_cfg_gene)]),
        "sp_hla_config_result_mapping": (_i32, [_vp, _u32, P(sp_hla_cfg_mapping)]),
        "sp_database_save_hla": (_i32, [_vp, _vp, _vp, _s, _s]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    for t in (sp_hla_alleles_stats, sp_hla_cfg_mapping, sp_hla_cfg_gene):
        if L.sp_struct_size(t.__name__.encode()) != C.sizeof(t):
            raise ImportError(f"{t.__name__} is {L.sp_struct_size(t.__name__.encode())} bytes in the library, {C.sizeof(t)} in this binding")
    _bound = True
    return L


def _b(x):
    return None if x is None else (x if isinstance(x, bytes) else str(x).encode())


def _d(x):
    return None if x is None else x.decode()


class Database:
    """sp_database: one database file (``.json`` / ``.json.gz`` path, or the bytes themselves)."""

    def __init__(self, source):
        self._h = _vp()
        err = C.create_string_buffer(512)
        if isinstance(source, (bytes, bytearray)):
            rc = _lib().sp_database_parse(bytes(source), len(source), C.byref(self._h), err, 512)
        else:
            rc = _lib().sp_database_load(_b(source), C.byref(self._h), err, 512)
        if rc != SP_OK:
            raise StarphaseError(rc, err.value.decode())

    def close(self):
        if self._h:
            _lib().sp_database_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != SP_OK:
            raise StarphaseError(rc, _lib().sp_database_last_error(self._h).decode())

    @property
    def metadata(self):
        m = sp_database_metadata()
        self._check(_lib().sp_database_get_metadata(self._h, C.byref(m)))
        return {k: getattr(m, k).decode() for k, _ in m._fields_}

    @property
    def stats(self):
        s = sp_database_stats()
        self._check(_lib().sp_database_info(self._h, C.byref(s)))
        return s

    def hla_genes(self):
        out = []
        for g in range(self.stats.n_hla_genes):
            r = sp_gene_region()
            self._check(_lib().sp_database_hla_gene(self._h, g, C.byref(r)))
            out.append(dict(name=r.name.decode(), chrom=r.chrom.decode(), start=r.start, end=r.end, is_forward_strand=bool(r.is_forward_strand),
                            is_absent_capable=bool(r.is_absent_capable), exons=[(r.exon_start[e], r.exon_end[e]) for e in range(r.n_exons)]))
        return out

    def gene_entries(self):
        out = []
        for i in range(self.stats.n_gene_entries):
            a, b = _s(), _s()
            self._check(_lib().sp_database_gene_entry(self._h, i, C.byref(a), C.byref(b)))
            out.append((a.value.decode(), b.value.decode()))
        return out

    def hla_flatten(self, gene_refs, genes=None, ref_buffer=100):
        """gene_refs: the hg38 bases of [start - ref_buffer, end + ref_buffer) per gene (in the order of `genes`, default: every gene of
        hla_config in name order).  Returns the sp_hla_db_desc (pointing into this database) and the allele names."""
        n = len(gene_refs)
        names = ffi._strs(genes) if genes is not None else None
        refs = ffi._strs(gene_refs)
        desc = sp_hla_db_desc()
        self._check(_lib().sp_database_hla_flatten(self._h, n, names, refs, ref_buffer, C.byref(desc)))
        alleles = []
        for i in range(desc.n_alleles):
            a, b, c = _s(), _s(), _s()
            self._check(_lib().sp_database_hla_allele(self._h, i, C.byref(a), C.byref(b), C.byref(c)))
            alleles.append((a.value.decode(), b.value.decode(), c.value.decode()))
        return desc, alleles

    def hla_db(self, ctx, gene_refs, genes=None, ref_buffer=100):
        """sp_database_hla_flatten + sp_hla_db_create -> (HlaDb, allele names)"""
        desc, alleles = self.hla_flatten(gene_refs, genes, ref_buffer)
        return ffi.HlaDb.from_desc(ctx, desc), alleles

    def cyp_window(self):
        c, a, b = _s(), _u64(), _u64()
        self._check(_lib().sp_database_cyp_window(self._h, C.byref(c), C.byref(a), C.byref(b)))
        return c.value.decode(), a.value, b.value

    def cyp_flatten(self, chrom_seq, window_start):
        self._cyp_seq = _b(chrom_seq)
        L, G, K = sp_cyp_locus(), sp_cyp_gene_def(), sp_cyp_config()
        self._check(_lib().sp_database_cyp_flatten(self._h, self._cyp_seq, int(window_start), len(self._cyp_seq), C.byref(L), C.byref(G), C.byref(K)))
        return L, G, K

    def cyp_db(self, ctx, chrom_seq, window_start):
        """sp_database_cyp_flatten + sp_cyp_db_create -> CypDb (ctx None: host tables only)"""
        L, G, K = self.cyp_flatten(chrom_seq, window_start)
        return ffi.CypDb.from_structs(ctx, L, G, K, keep=[self])

    def variant_gene(self, gene_name, chrom_seq=None):
        return VariantGene(self, gene_name, chrom_seq)

    def save_hla(self, alleles, result, hla_version, out_path):
        """sp_database_save_hla: this database with hla_sequences = `alleles` (HlaAlleles), hla_config = the genes of `result` (HlaConfigResult) and
        database_metadata.hla_version = hla_version, written to out_path (gzip when it ends in .gz)"""
        self._check(_lib().sp_database_save_hla(self._h, alleles._h, result._h, _b(hla_version), _b(out_path)))


class HlaAlleles:
    """sp_hla_alleles: the allele table of an IMGT/HLA release (hla_gen.fasta + hla_nuc.fasta, plain or gzip), in id order."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, gen, nuc):
        h = _vp()
        rc = _lib().sp_hla_fasta_load(_b(gen), _b(nuc), C.byref(h))
        if rc != SP_OK:
            raise StarphaseError(rc, _lib().sp_hla_fasta_last_error().decode())
        return cls(h)

    def close(self):
        if self._h:
            _lib().sp_hla_alleles_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stats(self):
        """dict(n_alleles, n_dna, n_dropped_no_cdna, n_dropped_gene, warnings)"""
        s = sp_hla_alleles_stats()
        rc = _lib().sp_hla_alleles_info(self._h, C.byref(s))
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_hla_alleles_info")
        return dict(n_alleles=s.n_alleles, n_dna=s.n_dna, n_dropped_no_cdna=s.n_dropped_no_cdna, n_dropped_gene=s.n_dropped_gene, warnings=s.warnings.decode())

    def __len__(self):
        return self.stats["n_alleles"]

    def allele(self, i):
        """dict(hla_id, gene_name, star_allele = list of fields, dna_sequence = str or None, cdna_sequence): HlaAlleleDefinition"""
        a = [_s() for _ in range(5)]
        rc = _lib().sp_hla_alleles_get(self._h, int(i), *[C.byref(x) for x in a])
        if rc != SP_OK:
            raise StarphaseError(rc, f"sp_hla_alleles_get({i})")
        return dict(hla_id=a[0].value.decode(), gene_name=a[1].value.decode(), star_allele=a[2].value.decode().split(":"),
                    dna_sequence=_d(a[3].value), cdna_sequence=a[4].value.decode())

    def table(self):
        """{hla_id: allele}: the database's hla_sequences"""
        return {a["hla_id"]: a for a in (self.allele(i) for i in range(len(self)))}


class HlaConfigResult:
    """sp_hla_config_result: what Context.hla_config_extend found (or a hand-made one: HlaConfigResult.make)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def make(cls, genes):
        """genes: [(name, start, end)]"""
        n = len(genes)
        names = ffi._strs([g[0] for g in genes])
        start, end = (_u64 * max(1, n))(*[g[1] for g in genes]), (_u64 * max(1, n))(*[g[2] for g in genes])
        h = _vp()
        rc = _lib().sp_hla_config_result_create(n, names, start, end, C.byref(h))
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_hla_config_result_create")
        return cls(h)

    def close(self):
        if self._h:
            _lib().sp_hla_config_result_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _info(self):
        n, m, w = _u32(), _u32(), _s()
        rc = _lib().sp_hla_config_result_info(self._h, C.byref(n), C.byref(m), C.byref(w))
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_hla_config_result_info")
        return n.value, m.value, w.value.decode()

    @property
    def warnings(self):
        return self._info()[2]

    def genes(self):
        """per gene, name order: dict(name, chrom, start, end, moved, is_absent_capable, worst_allele (index or None), worst = (len, nm, unmapped), n_dna_alleles, n_mapped)"""
        out = []
        for g in range(self._info()[0]):
            x = sp_hla_cfg_gene()
            rc = _lib().sp_hla_config_result_gene(self._h, g, C.byref(x))
            if rc != SP_OK:
                raise StarphaseError(rc, "sp_hla_config_result_gene")
            out.append(dict(name=x.name.decode(), chrom=x.chrom.decode(), start=x.start, end=x.end, moved=bool(x.moved), is_absent_capable=bool(x.is_absent_capable),
                            worst_allele=x.worst_allele if x.worst_allele >= 0 else None,
                            worst=(x.worst_len, x.worst_nm, x.worst_unmapped) if x.worst_allele >= 0 else None, n_dna_alleles=x.n_dna_alleles, n_mapped=x.n_mapped))
        return out

    def mappings(self):
        """per allele of the table: None, or dict(rev, nm, q_start, q_end, t_start, t_end); `overflow` lists the alleles reported as none for the band / their length"""
        out, self.overflow = [], []
        for a in range(self._info()[1]):
            m = sp_hla_cfg_mapping()
            rc = _lib().sp_hla_config_result_mapping(self._h, a, C.byref(m))
            if rc != SP_OK:
                raise StarphaseError(rc, "sp_hla_config_result_mapping")
            if m.status < 0:
                self.overflow.append(a)
            out.append(dict(rev=m.rev, nm=m.nm, q_start=m.q_start, q_end=m.q_end, t_start=m.t_start, t_end=m.t_end) if m.status == 1 else None)
        return out


class VariantGene:
    """sp_variant_gene: one gene entry, normalised (load_database_haplotypes)"""

    def __init__(self, db, gene_name, chrom_seq=None):
        self.db = db
        self._seq = _b(chrom_seq)
        self._h = _vp()
        db._check(_lib().sp_variant_gene_create(db._h, _b(gene_name), self._seq, len(self._seq) if self._seq else 0, C.byref(self._h)))
        self._keep = None

    def close(self):
        if self._h:
            _lib().sp_variant_gene_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != SP_OK:
            raise StarphaseError(rc, _lib().sp_variant_gene_last_error(self._h).decode())

    @property
    def stats(self):
        s = sp_variant_gene_stats()
        self._check(_lib().sp_variant_gene_info(self._h, C.byref(s)))
        return s

    def haplotypes(self):
        out = []
        for h in range(self.stats.n_haplotypes):
            a, b = _s(), _s()
            self._check(_lib().sp_variant_gene_haplotype(self._h, h, C.byref(a), C.byref(b)))
            out.append((a.value.decode(), _d(b.value)))
        return out

    def variants(self):
        out = []
        for v in range(self.stats.n_variants):
            pos, ref, alt, name, rs, vid, core = _u64(), _s(), _s(), _s(), _s(), _i64(), _i32()
            self._check(_lib().sp_variant_gene_variant(self._h, v, C.byref(pos), C.byref(ref), C.byref(alt), C.byref(name), C.byref(rs), C.byref(vid), C.byref(core)))
            out.append(dict(position=pos.value, ref=ref.value.decode(), alt=alt.value.decode(), name=name.value.decode(), dbsnp_id=_d(rs.value),
                            variant_id=vid.value, is_core_variant=bool(core.value)))
        return out

    def sv_definitions(self):
        d = sp_sv_definitions()
        self._check(_lib().sp_variant_gene_sv_definitions(self._h, C.byref(d)))
        return d

    def is_deletion(self, start, end):
        d = self.sv_definitions()
        kind, index = _i32(0), _i32(-1)
        rc = ffi.lib().sp_variant_is_deletion(C.byref(d), int(start), int(end), C.byref(kind), C.byref(index))
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_variant_is_deletion")
        if kind.value == 0:
            return None
        s = _s()
        self._check(_lib().sp_variant_gene_sv_label(self._h, kind.value, index.value, C.byref(s)))
        return s.value.decode()

    def problem(self, alleles=(), deletions=(), max_sv_length=0):
        """alleles: (position0, ref, alt, gt, ps|None) per ALT allele of a record; deletions: (start, end, gt, ps|None).
        Returns the sp_variant_problem (valid until the next call)."""
        A = (sp_vcf_allele * max(1, len(alleles)))()
        keep = []
        for i, (pos, ref, alt, gt, ps) in enumerate(alleles):
            keep += [_b(ref), _b(alt)]
            A[i] = sp_vcf_allele(int(pos), keep[-2], keep[-1], int(gt), 0, -1 if ps is None else int(ps))
        D = (sp_vcf_deletion * max(1, len(deletions)))()
        for i, (s, e, gt, ps) in enumerate(deletions):
            D[i] = sp_vcf_deletion(int(s), int(e), int(gt), 0, -1 if ps is None else int(ps))
        p = sp_variant_problem()
        self._check(_lib().sp_variant_gene_problem(self._h, len(alleles), A, len(deletions), D, int(max_sv_length), C.byref(p)))
        return p

    def problem_variant(self, vid):
        k, s, a, b = _i32(), _s(), _u64(), _u64()
        self._check(_lib().sp_variant_gene_problem_variant(self._h, int(vid), C.byref(k), C.byref(s), C.byref(a), C.byref(b)))
        return k.value, _d(s.value), a.value, b.value

    def problem_sv_label(self, label_id):
        s = _s()
        self._check(_lib().sp_variant_gene_problem_sv_label(self._h, int(label_id), C.byref(s)))
        return s.value.decode()


def problem_arrays(p):
    """the arrays of an sp_variant_problem as Python lists (tests compare them)"""
    def arr(ptr, n, t):
        return list(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(t)), (n,))) if n else []
    n_slots = arr(p.slot_off, p.n_haps + 1, C.c_int32)[-1] if p.n_haps >= 0 else 0
    alt_off = arr(p.alt_off, n_slots + 1, C.c_int32)
    return dict(n_haps=p.n_haps, hap_is_sv=arr(p.hap_is_sv, p.n_haps, C.c_uint8), hap_is_core=arr(p.hap_is_core, p.n_haps, C.c_uint8),
                slot_off=arr(p.slot_off, p.n_haps + 1, C.c_int32), alt_off=alt_off, alt_var=arr(p.alt_var, alt_off[-1], C.c_int32),
                n_vars=p.n_vars, var_is_core=arr(p.var_is_core, p.n_vars, C.c_uint8), n_obs=p.n_obs, obs_var=arr(p.obs_var, p.n_obs, C.c_int32),
                obs_gt=arr(p.obs_gt, p.n_obs, C.c_int32), obs_ps=arr(p.obs_ps, p.n_obs, C.c_int64), obs_sv_label=arr(p.obs_sv_label, p.n_obs, C.c_int32))


class GeneDetails:
    """sp_gene_details: the parts of one PgxGeneDetails"""

    def __init__(self):
        self._h = _vp()
        _lib().sp_gene_details_create(C.byref(self._h))

    def __del__(self):
        try:
            if self._h:
                _lib().sp_gene_details_free(self._h)
                self._h = _vp()
        except Exception:
            pass

    def add_diplotype(self, h1, h2):
        _lib().sp_gene_details_add_diplotype(self._h, _b(h1), _b(h2)); return self

    def add_simple_diplotype(self, h1, h2):
        _lib().sp_gene_details_add_simple_diplotype(self._h, _b(h1), _b(h2)); return self

    def set_simple_diplotypes(self, some):
        _lib().sp_gene_details_set_simple_diplotypes(self._h, 1 if some else 0); return self

    def add_inexact_diplotype(self, hap1, hap2):
        """hap = (base haplotype, [(label, is_vi, state), ...])"""
        args = []
        for base, rel in (hap1, hap2):
            labels = ffi._strs([r[0] for r in rel])
            vi = np.array([1 if r[1] else 0 for r in rel] or [0], np.uint8)
            st = np.array([r[2] for r in rel] or [0], np.int32)
            args += [_b(base), len(rel), labels, vi, st]
        a = args
        rc = _lib().sp_gene_details_add_inexact_diplotype(self._h, a[0], a[1], a[2], ffi._ptr(a[3]), ffi._ptr(a[4]), a[5], a[6], a[7], ffi._ptr(a[8]), ffi._ptr(a[9]))
        assert rc == SP_OK
        return self

    def add_diplotype_only(self, h1, h2):
        _lib().sp_gene_details_add_diplotype_only(self._h, _b(h1), _b(h2)); return self

    def add_variant(self, variant_id, name, dbsnp, chrom, position, ref, alt, genotype, phase_set=None, is_core=True, sv=None):
        v = sp_variant_detail(int(variant_id), _b(name), _b(dbsnp), _b(chrom), int(position), _b(ref), _b(alt), _b(sv[2]) if sv else None,
                              int(sv[0]) if sv else 0, int(sv[1]) if sv else 0, int(genotype), 1 if is_core else 0, -1 if phase_set is None else int(phase_set))
        rc = _lib().sp_gene_details_add_variant(self._h, C.byref(v))
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_gene_details_add_variant")
        return self

    @staticmethod
    def _stats(s):
        if s is None:
            return None
        seq_len, nm, unmapped = s[:3]
        clips = s[3:] if len(s) > 3 and s[3] is not None else None
        return sp_mapping_stats(1, 1 if clips else 0, int(seq_len), int(nm), int(unmapped), int(clips[0]) if clips else 0, int(clips[1]) if clips else 0)

    def add_mapping(self, qname, hla_id, star, cdna=None, dna=None, is_ignored=False):
        c, d = self._stats(cdna), self._stats(dna)
        _lib().sp_gene_details_add_mapping(self._h, _b(qname), _b(hla_id), _b(star), C.byref(c) if c else None, C.byref(d) if d else None, 1 if is_ignored else 0)
        return self

    def add_multi_mapping(self, qname, start, end, consensus_id, star):
        _lib().sp_gene_details_add_multi_mapping(self._h, _b(qname), int(start), int(end), int(consensus_id), _b(star)); return self


class Result:
    """sp_result: StarphaseJson"""

    def __init__(self, db=None, version=""):
        self._h = _vp()
        _lib().sp_result_create(db._h if db is not None else None, _b(version), C.byref(self._h))

    def __del__(self):
        try:
            if self._h:
                _lib().sp_result_free(self._h)
                self._h = _vp()
        except Exception:
            pass

    def _check(self, rc):
        if rc != SP_OK:
            raise StarphaseError(rc, _lib().sp_result_last_error(self._h).decode())

    def insert(self, gene, details, constructor):
        self._check(_lib().sp_result_insert(self._h, _b(gene), details._h if details is not None else None, int(constructor)))

    def json(self):
        s, n = _s(), _u64()
        self._check(_lib().sp_result_json(self._h, C.byref(s), C.byref(n)))
        return s.value.decode()

    def save(self, path):
        self._check(_lib().sp_result_save(self._h, _b(path)))

    def pharmcat_tsv(self):
        s, n = _s(), _u64()
        self._check(_lib().sp_result_pharmcat_tsv(self._h, C.byref(s), C.byref(n)))
        return s.value.decode()

    def save_pharmcat_tsv(self, path):
        self._check(_lib().sp_result_save_pharmcat_tsv(self._h, _b(path)))


# ------------------------------------------------------------------ debug files (sp_hla_debug_*, sp_aln_strings)
def aln_strings(aln, events, target):
    """sp_aln_strings: one row of Context.align_batch(..., events=True) (A = query, B = target) -> (cigar, md, match_len)"""
    a = ffi.sp_aln(*[int(aln[k]) for k in ("ok", "nm", "a_start", "a_end", "b_start", "b_end", "a_len", "b_len")])
    ev = np.ascontiguousarray(events, np.uint32)
    cap = 16 * (int(aln["nm"]) + 2) + 32
    cg, md, ml = C.create_string_buffer(cap), C.create_string_buffer(cap), _u64()
    rc = _lib().sp_aln_strings(C.byref(a), ev.ctypes.data, _b(target), len(target), cg, cap, md, cap, C.byref(ml))
    if rc != SP_OK:
        raise StarphaseError(rc, "sp_aln_strings")
    return cg.value.decode(), md.value.decode(), ml.value


def affine_cigar_strings(aln, cigar, target, cigar_cap=None, md_cap=None):
    """sp_affine_cigar_strings: one row of Context.affine_align / HlaDb.realign_cigars (aln: score, nm, a_start, a_end, b_start, b_end with a = query, b = target;
    cigar: its ops) -> (cigar string with M for '=' and 'X', md, match_len)"""
    a = np.array([tuple(int(aln[k]) for k in ("score", "nm", "a_start", "a_end", "b_start", "b_end"))], ffi.AFFINE_DTYPE)
    ops = np.ascontiguousarray(cigar, np.uint32)
    cap = 12 * (len(ops) + 2) + int(aln["b_end"]) - int(aln["b_start"]) + 32
    ccap, mcap = cigar_cap or cap, md_cap or cap
    cg, md, ml = C.create_string_buffer(ccap), C.create_string_buffer(mcap), _u64()
    rc = _lib().sp_affine_cigar_strings(a.ctypes.data, ops.ctypes.data, len(ops), _b(target), len(target), cg, ccap, md, mcap, C.byref(ml))
    if rc != SP_OK:
        raise StarphaseError(rc, "sp_affine_cigar_strings")
    return cg.value.decode(), md.value.decode(), ml.value


def affine_cigar_strings_eqx(aln, cigar, target, cigar_cap=None, md_cap=None):
    """sp_affine_cigar_strings_eqx: affine_cigar_strings with '=' and 'X' runs kept apart (the cigar of hla_debug.json's per-allele mappings)"""
    a = np.array([tuple(int(aln[k]) for k in ("score", "nm", "a_start", "a_end", "b_start", "b_end"))], ffi.AFFINE_DTYPE)
    ops = np.ascontiguousarray(cigar, np.uint32)
    cap = 12 * (len(ops) + 2) + int(aln["b_end"]) - int(aln["b_start"]) + 32
    ccap, mcap = cigar_cap or cap, md_cap or cap
    cg, md, ml = C.create_string_buffer(ccap), C.create_string_buffer(mcap), _u64()
    rc = _lib().sp_affine_cigar_strings_eqx(a.ctypes.data, ops.ctypes.data, len(ops), _b(target), len(target), cg, ccap, md, mcap, C.byref(ml))
    if rc != SP_OK:
        raise StarphaseError(rc, "sp_affine_cigar_strings_eqx")
    return cg.value.decode(), md.value.decode(), ml.value


def affine_detailed_mapping(aln, cigar, target, query_len):
    """DetailedMappingStats::from_mapping for such a row: a dict with the fields of sp_detailed_mapping"""
    cg, md, ml = affine_cigar_strings(aln, cigar, target)
    return dict(query_len=int(query_len), target_len=len(target), match_len=ml, nm=int(aln["nm"]), query_unmapped=int(query_len) - (int(aln["a_end"]) - int(aln["a_start"])),
                target_unmapped=len(target) - (int(aln["b_end"]) - int(aln["b_start"])), cigar=cg, md=md)


def detailed_mapping(aln, events, target):
    """DetailedMappingStats::from_mapping for one alignment row: a dict with the fields of sp_detailed_mapping"""
    cg, md, ml = aln_strings(aln, events, target)
    return dict(query_len=int(aln["a_len"]), target_len=int(aln["b_len"]), match_len=ml, nm=int(aln["nm"]),
                query_unmapped=int(aln["a_len"]) - (int(aln["a_end"]) - int(aln["a_start"])),
                target_unmapped=int(aln["b_len"]) - (int(aln["b_end"]) - int(aln["b_start"])), cigar=cg, md=md)


class HlaDebug:
    """sp_hla_debug: hla_debug.json"""

    def __init__(self):
        self._h = _vp()
        _lib().sp_hla_debug_create(C.byref(self._h))

    def close(self):
        if self._h:
            _lib().sp_hla_debug_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != SP_OK:
            raise StarphaseError(rc, _lib().sp_hla_debug_last_error(self._h).decode())

    @staticmethod
    def _dm(m):
        if m is None:
            return None, None
        keep = (_b(m["cigar"]), _b(m["md"]))
        return sp_detailed_mapping(1, 0, m["query_len"], m["target_len"], m["match_len"], m["nm"], m["query_unmapped"], m["target_unmapped"], *keep), keep

    def add_read(self, gene, qname, best_id=None, best_star=None):
        self._check(_lib().sp_hla_debug_add_read(self._h, _b(gene), _b(qname), _b(best_id), _b(best_star))); return self

    def add_mapping(self, gene, qname, hla_id, cdna=None, dna=None):
        c, _k1 = self._dm(cdna)
        d, _k2 = self._dm(dna)
        self._check(_lib().sp_hla_debug_add_mapping(self._h, _b(gene), _b(qname), _b(hla_id), C.byref(c) if c else None, C.byref(d) if d else None)); return self

    def add_dual_stats(self, gene, call):
        self._check(_lib().sp_hla_debug_add_dual_stats(self._h, _b(gene), C.byref(call))); return self

    def json(self):
        s, n = _s(), _u64()
        self._check(_lib().sp_hla_debug_json(self._h, C.byref(s), C.byref(n)))
        return s.value.decode()

    def save(self, path):
        self._check(_lib().sp_hla_debug_save(self._h, _b(path)))


# ------------------------------------------------------------------ input files (sp_bam_*, sp_vcf_*)
class sp_bam_read(C.Structure):
    _fields_ = [("qname", _s), ("flag", _u32), ("mapq", _u32), ("ref_id", _i32), ("reserved", _i32), ("pos", _i64), ("end", _i64),
                ("l_seq", _u32), ("n_cigar", _u32), ("cigar", C.POINTER(_u32))]


_io_bound = False


def _io():
    global _io_bound
    L = _lib()
    if _io_bound:
        return L
    P = C.POINTER
    sigs = {
        "sp_bam_open": (_i32, [_s, P(_vp), _s, _u32]),
        "sp_bam_free": (None, [_vp]),
        "sp_bam_last_error": (_s, [_vp]),
        "sp_bam_references": (_i32, [_vp, P(_u32), P(P(_s)), P(P(_u64))]),
        "sp_bam_fetch": (_i32, [_vp, _s, _u64, _u64, _u32, _i32, P(P(sp_bam_read)), P(_u32), P(_vp), P(P(_u64))]),
        "sp_bam_forget": (_i32, [_vp]),
        "sp_bam_last_seq4": (_i32, [_vp, P(_vp), P(P(_u64)), P(P(_u32)), P(_u32)]),
        "sp_vcf_open": (_i32, [_s, P(_vp), _s, _u32]),
        "sp_vcf_free": (None, [_vp]),
        "sp_vcf_index_info": (_i32, [_vp, P(_i32), P(_u64)]),
        "sp_vcf_last_error": (_s, [_vp]),
        "sp_vcf_samples": (_i32, [_vp, P(_u32), P(P(_s))]),
        "sp_vcf_alleles": (_i32, [_vp, _s, _s, _u64, _u64, P(P(sp_vcf_allele)), P(_u32)]),
        "sp_vcf_deletions": (_i32, [_vp, _s, _s, _u64, _u64, P(P(sp_vcf_deletion)), P(_u32)]),
        "sp_fasta_open": (_i32, [_s, P(_vp), _s, _u32]),
        "sp_fasta_free": (None, [_vp]),
        "sp_fasta_last_error": (_s, [_vp]),
        "sp_fasta_sequences": (_i32, [_vp, P(_u32), P(P(_s)), P(P(_u64))]),
        "sp_fasta_fetch": (_i32, [_vp, _s, _u64, _u64, P(_s), P(_u64)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _io_bound = True
    return L


class Bam:
    """sp_bam: an (indexed) BAM file"""

    def __init__(self, path):
        self._h = _vp()
        err = C.create_string_buffer(512)
        rc = _io().sp_bam_open(_b(path), C.byref(self._h), err, 512)
        if rc != SP_OK:
            raise StarphaseError(rc, err.value.decode())

    def __del__(self):
        try:
            if self._h:
                _io().sp_bam_free(self._h)
                self._h = _vp()
        except Exception:
            pass

    def references(self):
        n, names, lens = _u32(), C.POINTER(_s)(), C.POINTER(_u64)()
        _io().sp_bam_references(self._h, C.byref(n), C.byref(names), C.byref(lens))
        return [(names[i].decode(), int(lens[i])) for i in range(n.value)]

    def fetch(self, chrom, start, end, exclude_flags=0, dedupe=False):
        """-> list of dict(qname, flag, mapq, pos, end, cigar [(op, len)], seq)"""
        reads, n, bases, offs = C.POINTER(sp_bam_read)(), _u32(), _vp(), C.POINTER(_u64)()
        rc = _io().sp_bam_fetch(self._h, _b(chrom), int(start), int(end), int(exclude_flags), 1 if dedupe else 0, C.byref(reads), C.byref(n), C.byref(bases),
                                C.byref(offs))
        if rc != SP_OK:
            raise StarphaseError(rc, _io().sp_bam_last_error(self._h).decode())
        blob = C.string_at(bases.value, int(offs[n.value])) if n.value else b""
        out = []
        for i in range(n.value):
            r = reads[i]
            out.append(dict(qname=r.qname.decode(), flag=r.flag, mapq=r.mapq, pos=r.pos, end=r.end,
                            cigar=[(r.cigar[k] & 15, r.cigar[k] >> 4) for k in range(r.n_cigar)], seq=blob[offs[i]:offs[i + 1]].decode()))
        return out

    def last_seq4(self):
        """the SEQ fields of the last fetch as the file stores them -> (bytes as uint8 array, byte offsets[n + 1], lengths[n]): the arguments
        of Context.upload_format(SP_SEQ_BAM4, ...)"""
        import numpy as np
        seq, off, ln, n = _vp(), C.POINTER(_u64)(), C.POINTER(_u32)(), _u32()
        rc = _io().sp_bam_last_seq4(self._h, C.byref(seq), C.byref(off), C.byref(ln), C.byref(n))
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_bam_last_seq4")
        k = n.value
        offs = np.array([off[i] for i in range(k + 1)], np.uint64) if k else np.zeros(1, np.uint64)
        blob = np.frombuffer(C.string_at(seq.value, int(offs[-1])), np.uint8).copy() if k and offs[-1] else np.zeros(0, np.uint8)
        return blob, offs, np.array([ln[i] for i in range(k)], np.uint32)

    def forget(self):
        _io().sp_bam_forget(self._h)


class Vcf:
    """sp_vcf: a VCF file (plain, gzip or bgzip)"""

    def __init__(self, path):
        self._h = _vp()
        err = C.create_string_buffer(512)
        rc = _io().sp_vcf_open(_b(path), C.byref(self._h), err, 512)
        if rc != SP_OK:
            raise StarphaseError(rc, err.value.decode())

    def __del__(self):
        try:
            if self._h:
                _io().sp_vcf_free(self._h)
                self._h = _vp()
        except Exception:
            pass

    def _check(self, rc):
        if rc != SP_OK:
            raise StarphaseError(rc, _io().sp_vcf_last_error(self._h).decode())

    def index_info(self):
        """-> (read through a tabix / CSI index?, record lines the region fetches have parsed so far)"""
        ix, n = _i32(), _u64()
        _io().sp_vcf_index_info(self._h, C.byref(ix), C.byref(n))
        return bool(ix.value), int(n.value)

    def samples(self):
        n, names = _u32(), C.POINTER(_s)()
        _io().sp_vcf_samples(self._h, C.byref(n), C.byref(names))
        return [names[i].decode() for i in range(n.value)]

    def alleles(self, chrom, start=0, end=2 ** 62, sample=None):
        """-> [(position0, ref, alt, gt, ps|None)], the rows VariantGene.problem takes"""
        out, n = C.POINTER(sp_vcf_allele)(), _u32()
        self._check(_io().sp_vcf_alleles(self._h, _b(sample), _b(chrom), int(start), int(end), C.byref(out), C.byref(n)))
        return [(out[i].position, out[i].ref.decode(), out[i].alt.decode(), out[i].gt, None if out[i].ps < 0 else out[i].ps) for i in range(n.value)]

    def deletions(self, chrom, start=0, end=2 ** 62, sample=None):
        out, n = C.POINTER(sp_vcf_deletion)(), _u32()
        self._check(_io().sp_vcf_deletions(self._h, _b(sample), _b(chrom), int(start), int(end), C.byref(out), C.byref(n)))
        return [(out[i].start, out[i].end, out[i].gt, None if out[i].ps < 0 else out[i].ps) for i in range(n.value)]


class Fasta:
    """sp_fasta: the reference FASTA (plain with or without .fai, gzip)"""

    def __init__(self, path):
        self._h = _vp()
        err = C.create_string_buffer(512)
        rc = _io().sp_fasta_open(_b(path), C.byref(self._h), err, 512)
        if rc != SP_OK:
            raise StarphaseError(rc, err.value.decode())

    def __del__(self):
        try:
            if self._h:
                _io().sp_fasta_free(self._h)
                self._h = _vp()
        except Exception:
            pass

    def sequences(self):
        n, names, lens = _u32(), C.POINTER(_s)(), C.POINTER(_u64)()
        _io().sp_fasta_sequences(self._h, C.byref(n), C.byref(names), C.byref(lens))
        return [(names[i].decode(), lens[i]) for i in range(n.value)]

    def fetch(self, chrom, start, end):
        b, n = _s(), _u64()
        rc = _io().sp_fasta_fetch(self._h, _b(chrom), int(start), int(end), C.byref(b), C.byref(n))
        if rc != SP_OK:
            raise StarphaseError(rc, _io().sp_fasta_last_error(self._h).decode())
        return C.string_at(b, n.value).decode()


# ---------------------------------------------------------------- files to files (sp_starphase_*)
SETTINGS_STRINGS = ("include_set", "exclude_set", "sample_name", "sv_vcf", "debug_folder")


def settings_default():
    """sp_diplotype_settings_default() as a dict"""
    s = sp_diplotype_settings()
    _lib().sp_diplotype_settings_default(C.byref(s))
    return {k: (_d(getattr(s, k)) if k in SETTINGS_STRINGS else getattr(s, k)) for k, _t in sp_diplotype_settings._fields_}


def _settings(**kw):
    s = sp_diplotype_settings()
    _lib().sp_diplotype_settings_default(C.byref(s))
    for k, v in kw.items():
        if k not in dict(sp_diplotype_settings._fields_):
            raise KeyError(k)
        setattr(s, k, _b(v) if k in SETTINGS_STRINGS else v)
    return s


def _inputs(bams=(), vcf=None, sv_vcf=None, sample_name=None):
    arr = (_s * max(1, len(bams)))(*[_b(b) for b in bams])
    return sp_sample_inputs(len(bams), arr, _b(vcf), _b(sv_vcf), _b(sample_name)), arr


def settings_check(bams=(), vcf=None, **kw):
    """sp_diplotype_settings_check: (status, message, settings dict after the check)"""
    s = _settings(**kw)
    inp, _keep = _inputs(bams, vcf)
    err = C.create_string_buffer(512)
    rc = _lib().sp_diplotype_settings_check(C.byref(s), C.byref(inp), err, 512)
    return rc, err.value.decode(), {k: getattr(s, k) for k, _t in sp_diplotype_settings._fields_ if k not in SETTINGS_STRINGS}


class Starphase:
    """sp_starphase: a database + reference loaded once, sp_starphase_call per sample.  ctx: a Context or None (the handle makes its own).
    consensus_support=True: set_consensus_support() at once (a call with a debug folder also writes consensus_support.json); cyp_consensus_support=True:
    set_cyp_consensus_support() at once (it also writes cyp2d6_consensus_support.json); support_insertions=True: set_support_insertions() at once (those two files
    also list the inserted strings of the columns their insertions contest)."""

    def __init__(self, database, reference=None, ctx=None, consensus_support=False, cyp_consensus_support=False, support_insertions=False, support_haplotypes=False, hla_ties=False, cyp_vcf=False, cyp_alternatives=False, cyp_alternative_reads=False, variant_alternatives=False, **settings):
        self._h = _vp()
        self._s = _settings(**settings)
        rc = _lib().sp_starphase_create(ctx._h if ctx is not None else None, _b(database), _b(reference), C.byref(self._s), C.byref(self._h))
        if rc != SP_OK:
            raise StarphaseError(rc, _d(_lib().sp_starphase_last_error(None)))
        if consensus_support:
            self.set_consensus_support(True)
        if cyp_consensus_support:
            self.set_cyp_consensus_support(True)
        if support_insertions:
            self.set_support_insertions(True)
        if support_haplotypes:
            self.set_support_haplotypes(True)
        if hla_ties:
            self.set_hla_ties(True)
        if cyp_vcf:
            self.set_cyp_vcf(True)
        if cyp_alternatives:
            self.set_cyp_alternatives(True)
        if cyp_alternative_reads:
            self.set_cyp_alternative_reads(True)
        if variant_alternatives:
            self.set_variant_alternatives(True)

    def close(self):
        if self._h:
            _lib().sp_starphase_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_consensus_support(self, on=True):
        """sp_starphase_set_consensus_support: a debug folder also receives consensus_support.json (per HLA gene and consensus: how many member reads span, agree with or
        contest each consensus column); off by default"""
        rc = _lib().sp_starphase_set_consensus_support(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_consensus_support")
        return self

    def set_support_haplotypes(self, on=True):
        """sp_starphase_set_support_haplotypes: consensus_support.json and cyp2d6_consensus_support.json, where their own switches write them, also carry "haplotypes":
        the distinct patterns of calls the member reads make at the contested columns, with counts.  Off by default; no effect without one of those switches."""
        rc = _lib().sp_starphase_set_support_haplotypes(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_support_haplotypes")
        return self

    def set_support_insertions(self, on=True):
        """sp_starphase_set_support_insertions: consensus_support.json and cyp2d6_consensus_support.json, where their own switches write them, also carry "insertions":
        the inserted strings, with counts, behind every column that is contested by its insertions.  Off by default; no effect without one of those switches."""
        rc = _lib().sp_starphase_set_support_insertions(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_support_insertions")
        return self

    def set_cyp_vcf(self, on=True):
        """sp_starphase_set_cyp_vcf: a debug folder also receives cyp2d6_alleles.vcf.gz (one haploid sample per typed CYP2D6 region, one record per listed database variant,
        GT:SR:CR -- SR / CR: the member reads that span / agree with the consensus over the variant's window); off by default"""
        rc = _lib().sp_starphase_set_cyp_vcf(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_cyp_vcf")
        return self

    def set_cyp_alternatives(self, on=True):
        """sp_starphase_set_cyp_alternatives: a debug folder also receives cyp2d6_alternatives.json (the ten best CYP2D6 chain pairs, best first: diplotype, chains, score,
        its five components, edit distance, unmet observations and the coverage of each region); off by default"""
        rc = _lib().sp_starphase_set_cyp_alternatives(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_cyp_alternatives")
        return self

    def set_variant_alternatives(self, on=True):
        """sp_starphase_set_variant_alternatives: a debug folder also receives variant_alternatives.json (per solved variant gene the ten best diplotypes, best first:
        score, het combination, whether the call keeps it, and each haplotype's missing and unexpected variants); off by default"""
        rc = _lib().sp_starphase_set_variant_alternatives(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_variant_alternatives")
        return self

    def set_cyp_alternative_reads(self, on=True):
        """sp_starphase_set_cyp_alternative_reads: a debug folder also receives cyp2d6_alternative_reads.json (the ten best CYP2D6 chain pairs read by read: per pair
        the reads that are not neutral, with their excess edit distance, its difference to the call's, whether an observed chain of theirs is met and where they
        fit best; and the observed-chain table); off by default"""
        rc = _lib().sp_starphase_set_cyp_alternative_reads(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_cyp_alternative_reads")
        return self

    def set_cyp_consensus_support(self, on=True):
        """sp_starphase_set_cyp_consensus_support: a debug folder also receives cyp2d6_consensus_support.json (per CYP2D6 consensus region: how many member reads span,
        agree with or contest each column); off by default"""
        rc = _lib().sp_starphase_set_cyp_consensus_support(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_cyp_consensus_support")
        return self

    def set_hla_debug_mappings(self, on=True):
        """sp_starphase_set_hla_debug_mappings: hla_debug.json of a debug folder carries the mapping of each consensus against every allowed allele of its gene; off by default"""
        rc = _lib().sp_starphase_set_hla_debug_mappings(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_hla_debug_mappings")
        return self

    def set_hla_ties(self, on=True):
        """sp_starphase_set_hla_ties: a debug folder also receives hla_ties.json (per HLA gene and consensus: the alleles the call cannot tell from the winner of its
        a = 5 scan -- equal, score_only, beats_winner); off by default"""
        rc = _lib().sp_starphase_set_hla_ties(self._h, 1 if on else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_hla_ties")
        return self

    def set_read_debug(self, enable=True):
        """sp_starphase_set_read_debug: a debug folder also receives read_debug.json (every realigned HLA read's accepted allele with CIGAR and MD); off by default"""
        rc = _lib().sp_starphase_set_read_debug(self._h, 1 if enable else 0)
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_starphase_set_read_debug")
        return self

    def call(self, bams=(), vcf=None, sv_vcf=None, sample_name=None):
        """one sample -> Result"""
        inp, _keep = _inputs(bams, vcf, sv_vcf, sample_name)
        res = Result.__new__(Result)
        res._h = _vp()
        rc = _lib().sp_starphase_call(self._h, C.byref(inp), C.byref(res._h))
        if rc != SP_OK:
            raise StarphaseError(rc, _d(_lib().sp_starphase_last_error(self._h)))
        return res

    def call_batch(self, samples, max_group=None, threads=None, debug_folders=None):
        """sp_starphase_call_batch: samples = [dict(bams=..., vcf=..., sv_vcf=..., sample_name=...)] -> per sample a Result, or the StarphaseError
        that sample failed with (the others are still typed).  debug_folders: None or one folder (or None) per sample."""
        n = len(samples)
        keep = [_inputs(**smp) for smp in samples]
        inp = (sp_sample_inputs * max(1, n))(*[k[0] for k in keep])
        dbg = None
        if debug_folders is not None:
            if len(debug_folders) != n:
                raise ValueError("debug_folders: one entry per sample")
            dbg = (_s * max(1, n))(*[_b(d) for d in debug_folders])
        opts = sp_batch_options(max_group or 0, threads or 0)
        out = (_vp * max(1, n))()
        rcs = (_i32 * max(1, n))()
        rc = _lib().sp_starphase_call_batch(self._h, n, inp, dbg, C.byref(opts), out, rcs)
        if rc != SP_OK and not any(rcs[i] != SP_OK for i in range(n)):
            raise StarphaseError(rc, _d(_lib().sp_starphase_last_error(self._h)))
        res = []
        for i in range(n):
            if rcs[i] != SP_OK or not out[i]:
                res.append(StarphaseError(rcs[i], _d(_lib().sp_starphase_sample_error(self._h, i))))
                continue
            r = Result.__new__(Result)
            r._h = _vp(out[i])
            res.append(r)
        return res

    def sample_warnings(self, i):
        """the warnings of sample i of the last call_batch"""
        return _d(_lib().sp_starphase_sample_warnings(self._h, i))

    def batch_timing(self):
        t = sp_starphase_batch_timing()
        _lib().sp_starphase_last_batch_timing(self._h, C.byref(t))
        return {k: getattr(t, k) for k, _ty in sp_starphase_batch_timing._fields_ if k != "reserved_"}

    def warnings(self):
        return _d(_lib().sp_starphase_warnings(self._h))

    def timing(self):
        t = sp_starphase_timing()
        _lib().sp_starphase_last_timing(self._h, C.byref(t))
        return {k: getattr(t, k) for k, _ty in sp_starphase_timing._fields_}


def cli_path():
    """the `starphase_hip` executable the csrc Makefile builds next to the library"""
    import os
    return os.path.join(os.path.dirname(ffi.lib_path()), "starphase_hip")


def cyp_diplotype_cohort_mappings(cdb, read_sets, cap=None, **overrides):
    """sp_cyp_diplotype_cohort_mappings on a CypDb: per sample (sp_cyp_call, [(read, read_start, read_end, consensus, index_label)], status)"""
    pr = cdb.problem(**overrides)
    n = len(read_sets)
    calls = (ffi.sp_cyp_call * max(1, n))()
    handles = (_vp * max(1, n))(*[r._h.value if isinstance(r._h, C.c_void_p) else r._h for r in read_sets])
    cap = cap if cap is not None else sum(64 * r.n + 64 for r in read_sets)
    buf = (sp_cyp_read_mapping * max(1, cap))()
    off = (_u64 * (n + 1))()
    rcs = (_i32 * max(1, n))()
    rc = _lib().sp_cyp_diplotype_cohort_mappings(cdb.ctx._h, C.byref(pr), n, handles, calls, None, 0, None, buf, cap, off, rcs)
    if rc != SP_OK and not any(rcs[i] != SP_OK for i in range(n)):
        raise StarphaseError(rc, "sp_cyp_diplotype_cohort_mappings")
    return [(calls[i], [(m.read, m.read_start, m.read_end, m.consensus, m.index_label.decode()) for m in buf[off[i]:off[i + 1]]], rcs[i]) for i in range(n)]


def cyp_diplotype_mappings(cdb, reads, cap=None, **overrides):
    """sp_cyp_diplotype_mappings on a CypDb: (sp_cyp_call, [(read, read_start, read_end, consensus, index_label)])"""
    pr = cdb.problem(**overrides)
    call = ffi.sp_cyp_call()
    n = C.c_uint64(0)
    cap = cap if cap is not None else 64 * reads.n + 64
    buf = (sp_cyp_read_mapping * max(1, cap))()
    rc = _lib().sp_cyp_diplotype_mappings(cdb.ctx._h, C.byref(pr), reads._h, C.byref(call), None, 0, None, buf, cap, C.byref(n))
    if rc != SP_OK:
        raise StarphaseError(rc, "sp_cyp_diplotype_mappings")
    return call, [(m.read, m.read_start, m.read_end, m.consensus, m.index_label.decode()) for m in buf[:n.value]]


def cyp_call_with_consensus(cdb, reads, cons_cap=65536, **overrides):
    """sp_cyp_diplotype_mappings on a CypDb, keeping what sp_cyp_consensus_support takes: (sp_cyp_call, the consensus block (ctypes buffer of SP_CYP_MAXCONS * cons_cap
    bytes), [sp_cyp_read_mapping])"""
    return cyp_problem_call_with_consensus(cdb.ctx, cdb.problem(**overrides), reads, cons_cap)


def cyp_problem_call_with_consensus(ctx, pr, reads, cons_cap=65536):
    """the same on an sp_cyp_problem (ffi.Context.cyp_problem)"""
    call = ffi.sp_cyp_call()
    n = C.c_uint64(0)
    cap = 64 * reads.n + 64
    buf = (sp_cyp_read_mapping * max(1, cap))()
    cons = C.create_string_buffer(ffi.SP_CYP_MAXCONS * cons_cap)
    ctx.check(_lib().sp_cyp_diplotype_mappings(ctx._h, C.byref(pr), reads._h, C.byref(call), cons, cons_cap, None, buf, cap, C.byref(n)))
    return call, cons, [buf[i] for i in range(n.value)]


SP_CYP_VCF_FLANK = 2       # the default flank of a variant's window (include/starphase_hip.h)


def cyp_region_variants(has_variants, state):
    """an sp_cyp_region_variants from has_variants (up to SP_CYP_MAXCONS 0/1 entries) and state (uint8 [SP_CYP_MAXCONS, n_variants] or flat; kept alive by the record's
    `_state` attribute)"""
    import numpy as np
    rv = ffi.sp_cyp_region_variants()
    for h, x in enumerate(has_variants):
        rv.has_variants[h] = int(x)
    rv._state = np.ascontiguousarray(state, np.uint8)
    rv.state = rv._state.ctypes.data_as(_vp).value if rv._state.size else None
    return rv


def cyp_call_with_variants(cdb, reads, cons_cap=65536, **overrides):
    """sp_cyp_diplotype_mappings on a CypDb, keeping what sp_cyp_variant_support takes: (sp_cyp_problem, sp_cyp_call, consensus block, sp_cyp_region_variants,
    [sp_cyp_read_mapping])"""
    import numpy as np
    pr = cdb.problem(**overrides)
    call = ffi.sp_cyp_call()
    n = C.c_uint64(0)
    cap = 64 * reads.n + 64
    buf = (sp_cyp_read_mapping * max(1, cap))()
    cons = C.create_string_buffer(ffi.SP_CYP_MAXCONS * cons_cap)
    rv = cyp_region_variants([], np.full(ffi.SP_CYP_MAXCONS * max(1, pr.n_variants), 255, np.uint8))
    cdb.ctx.check(_lib().sp_cyp_diplotype_mappings(cdb.ctx._h, C.byref(pr), reads._h, C.byref(call), cons, cons_cap, C.byref(rv), buf, cap, C.byref(n)))
    return pr, call, cons, rv, [buf[i] for i in range(n.value)]


def cyp_variant_windows(aln, cigar, var_pos, var_ref_len, flank=SP_CYP_VCF_FLANK):
    """sp_cyp_variant_windows (host only): aln = one AFFINE_DTYPE record (consensus = query a, backbone = target b), cigar = its ops -> [(start, end) or None per variant]"""
    import numpy as np
    a = np.ascontiguousarray(aln, ffi.AFFINE_DTYPE).reshape(1)
    ops = np.ascontiguousarray(cigar, np.uint32)
    pos = np.ascontiguousarray(var_pos, np.int32)
    rl = np.ascontiguousarray(var_ref_len, np.uint32)
    win = np.zeros(max(1, len(pos)), ffi.WINDOW_DTYPE)
    ok = np.zeros(max(1, len(pos)), np.int32)
    rc = _lib().sp_cyp_variant_windows(ffi._ptr(a), ffi._ptr(ops), len(ops), len(pos), ffi._ptr(pos), ffi._ptr(rl), int(flank), ffi._ptr(win), ffi._ptr(ok))
    if rc != SP_OK:
        raise StarphaseError(rc, "sp_cyp_variant_windows")
    return [(int(win[v]["start"]), int(win[v]["end"])) if ok[v] else None for v in range(len(pos))]


def cyp_variant_support(ctx, pr, reads, call, cons, cons_cap, rv, mappings, flank=SP_CYP_VCF_FLANK, table=False):
    """sp_cyp_variant_support: what cyp_call_with_variants returned -> (support WINDOW_SUPPORT_DTYPE [SP_CYP_MAXCONS, n_variants], valid int32 of that shape); table=True
    adds what cyp_consensus_support returns ([cols per consensus], [summary dict per consensus]) from the same member pass"""
    import numpy as np
    NV = int(pr.n_variants)
    sup = np.zeros((ffi.SP_CYP_MAXCONS, max(1, NV)), ffi.WINDOW_SUPPORT_DTYPE)
    ok = np.zeros((ffi.SP_CYP_MAXCONS, max(1, NV)), np.int32)
    arr = _mapping_array(mappings)
    H = max(0, min(call.n_consensus, ffi.SP_CYP_MAXCONS))
    off = cols = sm = None
    total = 0
    if table:
        off = np.zeros(ffi.SP_CYP_MAXCONS + 1, np.uint64)
        total = sum(len(cyp_consensus_of(cons, cons_cap, h)) for h in range(H)) if call.status == 0 else 0
        cols = np.zeros(max(1, total), ffi.PILEUP_DTYPE)
        sm = np.zeros(ffi.SP_CYP_MAXCONS, ffi.SUPPORT_DTYPE)
    ctx.check(_lib().sp_cyp_variant_support(ctx._h, C.byref(pr), reads._h, C.byref(call), C.cast(cons, _vp), cons_cap, C.byref(rv), arr, len(mappings), int(flank),
                                            ffi._ptr(sup), ffi._ptr(ok), ffi._ptr(off), ffi._ptr(cols), total, ffi._ptr(sm)))
    sup, ok = sup[:, :NV], ok[:, :NV]
    if not table:
        return sup, ok
    return sup, ok, ([cols[int(off[h]):int(off[h + 1])].copy() for h in range(H)], [{n: int(sm[h][n]) for n in ffi.SUPPORT_FIELDS[:-1]} for h in range(H)])


def cyp_alleles_vcf(cdb, call, rv, support=None, support_valid=None, file_date=None, command=None, cap=None):
    """sp_cyp_alleles_vcf (host only): the text of cyp2d6_alleles.vcf.gz.  support / support_valid: [SP_CYP_MAXCONS, n_variants] as cyp_variant_support returned them.
    cap: a capacity to try, once -> (status, text, needed)"""
    import numpy as np
    sup = np.ascontiguousarray(support, ffi.WINDOW_SUPPORT_DTYPE) if support is not None else None
    ok = np.ascontiguousarray(support_valid, np.int32) if support_valid is not None else None
    need = _u64(0)
    args = (cdb._h, C.byref(call), C.byref(rv) if rv is not None else None, ffi._ptr(sup), ffi._ptr(ok), _b(file_date) if file_date is not None else None,
            _b(command) if command is not None else None)
    if cap is not None:
        buf = C.create_string_buffer(max(1, int(cap)))
        rc = _lib().sp_cyp_alleles_vcf(*args, buf, int(cap), C.byref(need))
        return rc, buf.value.decode(), need.value
    rc = _lib().sp_cyp_alleles_vcf(*args, None, 0, C.byref(need))
    if rc not in (SP_OK, ffi.SP_ERR_CAPACITY):
        raise StarphaseError(rc, "sp_cyp_alleles_vcf")
    buf = C.create_string_buffer(need.value)
    rc = _lib().sp_cyp_alleles_vcf(*args, buf, need.value, C.byref(need))
    if rc != SP_OK:
        raise StarphaseError(rc, "sp_cyp_alleles_vcf")
    return buf.value.decode()


def cyp_alleles_vcf_save(cdb, call, rv, path, support=None, support_valid=None, file_date=None, command=None):
    """sp_cyp_alleles_vcf_save: the text of cyp_alleles_vcf as a BGZF file"""
    import numpy as np
    sup = np.ascontiguousarray(support, ffi.WINDOW_SUPPORT_DTYPE) if support is not None else None
    ok = np.ascontiguousarray(support_valid, np.int32) if support_valid is not None else None
    rc = _lib().sp_cyp_alleles_vcf_save(cdb._h, C.byref(call), C.byref(rv) if rv is not None else None, ffi._ptr(sup), ffi._ptr(ok),
                                        _b(file_date) if file_date is not None else None, _b(command) if command is not None else None, _b(path))
    if rc != SP_OK:
        raise StarphaseError(rc, "sp_cyp_alleles_vcf_save")


def bgzf_save(path, data):
    """sp_bgzf_save: bytes -> a BGZF file"""
    data = bytes(data)
    rc = _lib().sp_bgzf_save(_b(path), C.cast(C.c_char_p(data), _vp), len(data))
    if rc != SP_OK:
        raise StarphaseError(rc, "sp_bgzf_save")


def cyp_consensus_of(cons, cons_cap, h):
    """consensus h of a consensus block, as text"""
    return cons.raw[h * cons_cap:(h + 1) * cons_cap].split(b"\0", 1)[0].decode()


def _mapping_array(mappings):
    arr = (sp_cyp_read_mapping * max(1, len(mappings)))()
    for i, m in enumerate(mappings):
        arr[i] = m
    return arr


def cyp_consensus_support(ctx, reads, call, cons, cons_cap, mappings, want_cols=True, insertions=False, haplotypes=False):
    """sp_cyp_consensus_support: call / cons / mappings as cyp_call_with_consensus returned them -> ([cols PILEUP_DTYPE per consensus] or None, [summary dict per consensus]).
    insertions=True (sp_cyp_consensus_support_ins) adds the INS_DTYPE records (col: consensus h's columns from the sum of the lengths before it) as a third item;
    haplotypes=True (sp_cyp_consensus_support_hap) adds, last, (HAP_DTYPE records, HAP_HEAD_DTYPE per consensus): target h, first_pair the member's mapping record"""
    import numpy as np
    H = max(0, min(call.n_consensus, ffi.SP_CYP_MAXCONS))
    off = np.zeros(ffi.SP_CYP_MAXCONS + 1, np.uint64)
    total = sum(len(cyp_consensus_of(cons, cons_cap, h)) for h in range(H)) if call.status == 0 else 0
    cols = np.zeros(max(1, total), ffi.PILEUP_DTYPE) if want_cols else None
    sm = np.zeros(ffi.SP_CYP_MAXCONS, ffi.SUPPORT_DTYPE)
    arr = _mapping_array(mappings)
    ins = None
    if haplotypes:
        n_i = _u64(0)
        ibuf = [np.zeros(16384, ffi.INS_DTYPE) if insertions else None]

        def run(haps, cap, n, heads):
            rc = _lib().sp_cyp_consensus_support_hap(ctx._h, reads._h, C.byref(call), C.cast(cons, _vp), cons_cap, arr, len(mappings), ffi._ptr(off), ffi._ptr(cols), total, ffi._ptr(sm),
                                                     ffi._ptr(ibuf[0]), len(ibuf[0]) if insertions else 0, C.byref(n_i) if insertions else None, haps, cap, n, heads)
            if insertions and rc == ffi.SP_ERR_CAPACITY and n_i.value > len(ibuf[0]):
                ibuf[0] = np.zeros(n_i.value, ffi.INS_DTYPE)
                return run(haps, cap, n, heads)
            return rc
        hap = ctx._with_haps(run, 4096, ffi.SP_CYP_MAXCONS)
        hap = (hap[0], hap[1][:H].copy())
        ins = ibuf[0][:n_i.value].copy() if insertions else None
    elif insertions:
        ins = ctx._with_ins(lambda ins, cap, n: _lib().sp_cyp_consensus_support_ins(ctx._h, reads._h, C.byref(call), C.cast(cons, _vp), cons_cap, arr, len(mappings), ffi._ptr(off),
                                                                                    ffi._ptr(cols), total, ffi._ptr(sm), ins, cap, n), 16384)
    else:
        ctx.check(_lib().sp_cyp_consensus_support(ctx._h, reads._h, C.byref(call), C.cast(cons, _vp), cons_cap, arr, len(mappings), ffi._ptr(off), ffi._ptr(cols), total, ffi._ptr(sm)))
    res = ([cols[int(off[h]):int(off[h + 1])].copy() for h in range(H)] if want_cols else None,
           [{n: int(sm[h][n]) for n in ffi.SUPPORT_FIELDS[:-1]} for h in range(H)])
    res = res + (ins,) if insertions else res
    return res + (hap,) if haplotypes else res


def cyp_consensus_support_cohort(ctx, read_sets, calls, cons_blocks, cons_cap, mapping_lists, insertions=False, haplotypes=False):
    """sp_cyp_consensus_support_cohort: per sample what cyp_call_with_consensus returned -> per sample ([cols per consensus], [summary dict per consensus]).
    insertions=True (sp_cyp_consensus_support_cohort_ins): -> (that, INS_DTYPE records, col_offset uint64[n * SP_CYP_MAXCONS + 1])"""
    import numpy as np
    n = len(read_sets)
    M = ffi.SP_CYP_MAXCONS
    carr = (ffi.sp_cyp_call * n)()
    for i, c in enumerate(calls):
        C.memmove(C.byref(carr[i]), C.byref(c), C.sizeof(ffi.sp_cyp_call))
    block = C.create_string_buffer(b"".join(b.raw for b in cons_blocks), n * M * cons_cap)
    flat = [m for ms in mapping_lists for m in ms]
    moff = np.zeros(n + 1, np.uint64)
    moff[1:] = np.cumsum([len(ms) for ms in mapping_lists])
    handles = (_vp * n)(*[r._h.value if isinstance(r._h, C.c_void_p) else r._h for r in read_sets])
    off = np.zeros(n * M + 1, np.uint64)
    total = sum(len(cyp_consensus_of(cons_blocks[i], cons_cap, h)) for i in range(n) if calls[i].status == 0 for h in range(max(0, min(calls[i].n_consensus, M))))
    cols = np.zeros(max(1, total), ffi.PILEUP_DTYPE)
    sm = np.zeros(n * M, ffi.SUPPORT_DTYPE)
    marr = _mapping_array(flat)
    ins = None
    if haplotypes:
        # sp_cyp_consensus_support_cohort_hap: -> (that, INS_DTYPE records or None, col_offset, (HAP_DTYPE records, HAP_HEAD_DTYPE per slot sample * SP_CYP_MAXCONS + h))
        n_i = _u64(0)
        ibuf = [np.zeros(16384, ffi.INS_DTYPE) if insertions else None]

        def run(haps, hcap, k, heads):
            rc = _lib().sp_cyp_consensus_support_cohort_hap(ctx._h, n, handles, carr, C.cast(block, _vp), cons_cap, marr, ffi._ptr(moff), ffi._ptr(off), ffi._ptr(cols), total, ffi._ptr(sm),
                                                            ffi._ptr(ibuf[0]), len(ibuf[0]) if insertions else 0, C.byref(n_i) if insertions else None, haps, hcap, k, heads)
            if insertions and rc == ffi.SP_ERR_CAPACITY and n_i.value > len(ibuf[0]):
                ibuf[0] = np.zeros(n_i.value, ffi.INS_DTYPE)
                return run(haps, hcap, k, heads)
            return rc
        hap = ctx._with_haps(run, 16384, n * M)
        ins = ibuf[0][:n_i.value].copy() if insertions else None
    elif insertions:
        ins = ctx._with_ins(lambda ins, cap, k: _lib().sp_cyp_consensus_support_cohort_ins(ctx._h, n, handles, carr, C.cast(block, _vp), cons_cap, marr, ffi._ptr(moff), ffi._ptr(off),
                                                                                           ffi._ptr(cols), total, ffi._ptr(sm), ins, cap, k), 16384)
    else:
        ctx.check(_lib().sp_cyp_consensus_support_cohort(ctx._h, n, handles, carr, C.cast(block, _vp), cons_cap, marr, ffi._ptr(moff), ffi._ptr(off), ffi._ptr(cols), total, ffi._ptr(sm)))
    out = []
    for i in range(n):
        H = max(0, min(calls[i].n_consensus, M)) if calls[i].status == 0 else 0
        out.append(([cols[int(off[i * M + h]):int(off[i * M + h + 1])].copy() for h in range(H)], [{k: int(sm[i * M + h][k]) for k in ffi.SUPPORT_FIELDS[:-1]} for h in range(H)]))
    if haplotypes:
        return out, ins, off.copy(), hap
    return (out, ins, off.copy()) if insertions else out


def cyp_support_json(call, consensus, cols, summaries, cap=None, insertions=None, mappings=None, read_names=None, haplotypes=None):
    """sp_cyp_support_json (host only): consensus = [text per consensus], cols = [PILEUP_DTYPE per consensus], summaries = [dict per consensus] -> the text of
    cyp2d6_consensus_support.json.  cap: a buffer size to try -> (status, text, needed).  insertions (INS_DTYPE; mappings and read_names optional, for first_read):
    sp_cyp_support_json_ins; haplotypes = (HAP_DTYPE records, HAP_HEAD_DTYPE per consensus): sp_cyp_support_json_hap"""
    import numpy as np
    H = len(consensus)
    cons_cap = max([len(s) for s in consensus] + [0]) + 1
    block = C.create_string_buffer(b"".join(s.encode().ljust(cons_cap, b"\0") for s in consensus), max(1, H * cons_cap))
    off = np.zeros(H + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in cols]) if H else 0
    table = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(c, ffi.PILEUP_DTYPE) for c in cols]) if H else np.zeros(0, ffi.PILEUP_DTYPE), ffi.PILEUP_DTYPE)
    if not len(table):
        table = np.zeros(1, ffi.PILEUP_DTYPE)
    sm = np.zeros(max(1, H), ffi.SUPPORT_DTYPE)
    for h, d in enumerate(summaries):
        for k in ffi.SUPPORT_FIELDS[:-1]:
            sm[h][k] = int(d.get(k, 0))
    need = _u64(0)
    args = (C.byref(call), C.cast(block, _vp), cons_cap, ffi._ptr(off), ffi._ptr(table), ffi._ptr(sm))
    if haplotypes is not None:
        ins = np.ascontiguousarray(insertions if insertions is not None else np.zeros(0, ffi.INS_DTYPE), ffi.INS_DTYPE)
        haps, heads = np.ascontiguousarray(haplotypes[0], ffi.HAP_DTYPE), np.ascontiguousarray(haplotypes[1], ffi.HAP_HEAD_DTYPE)
        marr = _mapping_array(mappings) if mappings is not None else None
        names, n_names = ffi._name_array(read_names)
        more = (ffi._ptr(ins) if len(ins) else None, len(ins), ffi._ptr(haps) if len(haps) else None, len(haps), ffi._ptr(heads) if len(heads) else None, 0,
                marr, len(mappings) if mappings is not None else 0, names, n_names)
        rc = _lib().sp_cyp_support_json_hap(*args, *more, None, 0, C.byref(need))
        if rc not in (SP_OK, ffi.SP_ERR_CAPACITY):
            raise StarphaseError(rc, "sp_cyp_support_json_hap")
        buf = C.create_string_buffer(need.value)
        rc = _lib().sp_cyp_support_json_hap(*args, *more, buf, need.value, C.byref(need))
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_cyp_support_json_hap")
        return buf.value.decode()
    if insertions is not None:
        ins = np.ascontiguousarray(insertions, ffi.INS_DTYPE)
        marr = _mapping_array(mappings) if mappings is not None else None
        names, n_names = ffi._name_array(read_names)
        need = _u64(0)
        more = (ffi._ptr(ins) if len(ins) else None, len(ins), marr, len(mappings) if mappings is not None else 0, names, n_names)
        rc = _lib().sp_cyp_support_json_ins(*args, *more, None, 0, C.byref(need))
        if rc not in (SP_OK, ffi.SP_ERR_CAPACITY):
            raise StarphaseError(rc, "sp_cyp_support_json_ins")
        buf = C.create_string_buffer(need.value)
        rc = _lib().sp_cyp_support_json_ins(*args, *more, buf, need.value, C.byref(need))
        if rc != SP_OK:
            raise StarphaseError(rc, "sp_cyp_support_json_ins")
        return buf.value.decode()
    if cap is not None:
        buf = C.create_string_buffer(max(1, cap))
        rc = _lib().sp_cyp_support_json(*args, buf if cap else None, cap, C.byref(need))
        return rc, buf.value.decode() if cap else "", need.value
    rc = _lib().sp_cyp_support_json(*args, None, 0, C.byref(need))
    if rc not in (SP_OK, ffi.SP_ERR_CAPACITY):
        raise StarphaseError(rc, "sp_cyp_support_json")
    buf = C.create_string_buffer(need.value)
    rc = _lib().sp_cyp_support_json(*args, buf, need.value, C.byref(need))
    if rc != SP_OK:
        raise StarphaseError(rc, "sp_cyp_support_json")
    return buf.value.decode()
