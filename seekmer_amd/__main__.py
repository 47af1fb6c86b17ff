#!/usr/bin/env python3
"""CLI (reference: seekmer/__main__.py:13-71): `seekmer_amd [--debug] {index,infer,infer-many,impute} ...`"""
import argparse
import logging
import sys

from . import impute
from . import index_builder
from . import infer


def make_parser():
    parser = argparse.ArgumentParser(prog='seekmer_amd', description='A fast RNA-seq tool',
                                     formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('-v', '--version', action='version', version='Seekmer 2019.0.0 (MI355X)')
    parser.add_argument('--debug', action='store_true', help='enable debugging messages')
    subparsers = parser.add_subparsers(title='subcommand', dest='subcommand')
    index_builder.add_subcommand_parser(subparsers)
    infer.add_subcommand_parser(subparsers)
    infer.add_many_subcommand_parser(subparsers)
    impute.add_subcommand_parser(subparsers)
    return parser


def parse_args(argv=None, parser=None):
    """The command line as the options a subcommand's run() takes; exits on a command line that cannot be."""
    parser = parser or make_parser()
    opts = vars(parser.parse_args(argv))
    if opts['subcommand'] in ('infer', 'infer-many', 'impute'):
        infer.length_model_option(parser, opts)
    if opts['subcommand'] in ('infer', 'infer-many'):
        infer.gene_option(opts)
    if opts['subcommand'] == 'infer-many':
        infer.barcode_option(parser, opts)
    return opts


def main(argv=None):
    parser = make_parser()
    opts = parse_args(argv, parser)
    logging.basicConfig(level=logging.DEBUG if opts['debug'] else logging.INFO,
                        format='%(levelname)-5s %(asctime)s %(name)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S', stream=sys.stderr)
    if opts['subcommand'] == 'index':
        index_builder.run(**opts)
    elif opts['subcommand'] == 'infer':
        infer.run(**opts)
    elif opts['subcommand'] == 'infer-many':
        infer.run_many(**opts)
    elif opts['subcommand'] == 'impute':
        impute.run(**opts)
    else:
        parser.print_help()
    return 0


if __name__ == '__main__':
    sys.exit(main())
