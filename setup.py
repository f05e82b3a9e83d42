"""Packaging of seekr_amd.  The HIP library is built in-tree first: `python -m seekr_amd.build`."""
from setuptools import setup

setup(
    name="seekr_amd",
    version="0.1.0",
    description="MI355X-native k-mer counting + Pearson hot path with SEEKR's API",
    packages=["seekr_amd"],
    package_data={"seekr_amd": ["libseekr_hip.so", "csrc/*"]},
    install_requires=["numpy"],
    extras_require={"csv": ["pandas"], "progress": ["tqdm"]},
    entry_points={
        "console_scripts": [
            # same command names as the reference (setup.py:63-65)
            "seekr_kmer_counts = seekr_amd.console_scripts:console_kmer_counts",
            "seekr_pearson = seekr_amd.console_scripts:console_pearson",
            "seekr_norm_vectors = seekr_amd.console_scripts:console_norm_vectors",
            "seekr_adj_pval = seekr_amd.console_scripts:console_adj_pval",
            "seekr_find_dist = seekr_amd.console_scripts:console_find_dist",
            "seekr_find_pval = seekr_amd.console_scripts:console_find_pval",
            # sliding windows of a target against queries (no counterpart in the reference)
            "seekr_domain_pearson = seekr_amd.console_scripts:console_domain_pearson",
            # the k most correlated rows of every row, without the all-pairs matrix (no counterpart either)
            "seekr_nearest = seekr_amd.console_scripts:console_nearest",
            # reciprocal nearest neighbours of two sets (or one) from one sweep (no counterpart either)
            "seekr_reciprocal_hits = seekr_amd.console_scripts:console_reciprocal_hits",
            # the pairs with a corrected p-value <= alpha, without r, p or the corrected matrix (no counterpart either)
            "seekr_significant_pairs = seekr_amd.console_scripts:console_significant_pairs",
            # the windows of a target each query is significantly similar to (no counterpart either)
            "seekr_domain_significant = seekr_amd.console_scripts:console_domain_significant",
            # hot windows of a target merged into intervals per query (no counterpart either)
            "seekr_domain_hits = seekr_amd.console_scripts:console_domain_hits",
            "seekr_kmer_leiden = seekr_amd.console_scripts:console_kmer_leiden",
            "seekr_pair_kmers = seekr_amd.console_scripts:console_pair_kmers",
            # histogram, exact quantiles and density cutoffs of r, without the all-pairs matrix (no counterpart either)
            "seekr_r_distribution = seekr_amd.console_scripts:console_r_distribution",
        ]
    },
)
